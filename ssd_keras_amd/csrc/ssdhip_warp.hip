// ssdhip_warp.hip -- cv2.warpAffine on 8-bit images (INTER_LINEAR, BORDER_CONSTANT) for a whole batch: the pixel half of the reference's
// Translate / Scale / Rotate (data_generator/object_detection_2d_geometric_ops.py:233-772) and of the constant-input-size chain.
//
// OpenCV 3.4 / 4.x up to 4.10 (modules/imgproc/src/imgwarp.cpp, WarpAffineInvoker + remapBilinear): the inverse matrix is turned into
// per-column (adelta, bdelta) = cvRound(M0 x 1024), cvRound(M3 x 1024) and per-row (X0, Y0) = cvRound((M1 y + M2) 1024) + 16, ... tables
// -- built on the host in NumPy (data_generator/_image_ops.warp_tables), so the device does integer arithmetic only:
//   X = (X0 + adelta) >> 5, (sx, fx) = (sat_short(X >> 5), X & 31), likewise Y;
//   out = sat_u8((sum_k w_k s_k + (1 << 14)) >> 15), w = 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy;
//   a neighbour outside the image reads the constant border value.
// Around the warp each image carries an integer translation before it (pre) and after it (post) and a horizontal flip, so a chain's
// Translate -> Scale -> Flip or Scale -> Translate -> Flip is ONE pass: an integer translation is an exact copy under this arithmetic
// (fx = fy = 0, weight 32768) with the border value where it uncovers the canvas.
//
// One thread writes four adjacent output pixels (4 C bytes: C dword stores when the row allows it); each source row pair of a pixel is
// one unaligned 8-byte load when both neighbours are inside (gfx950 runs with unaligned global access), byte loads at the edges.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"

namespace ssdhip {

typedef uint64_t __attribute__((aligned(1))) u64_unaligned;

struct WarpGeo {
    int flip, pre_dx, pre_dy, post_dx, post_dy;
};

// the C bytes of the pixel at byte offset `off` and of the one right of it, as two packed words (byte k = channel k)
template <int C>
__device__ __forceinline__ void load_pair(const unsigned char* __restrict__ x, long long off, long long total, bool left_in, bool right_in,
                                          unsigned bg, unsigned& a, unsigned& b) {
    if (left_in && right_in && off + 8 <= total) {
        const uint64_t v = *reinterpret_cast<const u64_unaligned*>(x + off);
        a = (unsigned)(v & ((C == 4) ? 0xffffffffull : ((1ull << (8 * C)) - 1)));
        b = (unsigned)((v >> (8 * C)) & ((C == 4) ? 0xffffffffull : ((1ull << (8 * C)) - 1)));
        return;
    }
    a = bg;
    b = bg;
    if (left_in) {
        unsigned v = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) v |= (unsigned)x[off + c] << (8 * c);
        a = v;
    }
    if (right_in) {
        unsigned v = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) v |= (unsigned)x[off + C + c] << (8 * c);
        b = v;
    }
}

template <int C>
__global__ __launch_bounds__(256) void warp_affine_u8_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W,
                                                             int Ho, int Wo, const int* __restrict__ geo, const int* __restrict__ xtab,
                                                             const int* __restrict__ ytab, const unsigned char* __restrict__ background,
                                                             long long total) {
    const int b = blockIdx.y;
    const int quads = (Wo + 3) >> 2;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)quads * Ho) return;
    const int oy = (int)(q / quads);
    const int ox0 = (int)(q - (long long)oy * quads) * 4;
    const int* g = geo + b * 5;
    const WarpGeo gg = {g[0], g[1], g[2], g[3], g[4]};
    unsigned bg = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) bg |= (unsigned)background[b * C + c] << (8 * c);
    const unsigned char* src = x + (long long)b * H * W * C;
    const long long src_off = (long long)b * H * W * C;
    const int* xt = xtab + (long long)b * Wo * 2;
    const int* yt = ytab + (long long)b * Ho * 2;

    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ox = ox0 + k;
        unsigned out = bg;
        const int x1 = gg.flip ? Wo - 1 - ox : ox;
        const int u = x1 - gg.post_dx, v = oy - gg.post_dy;
        if (ox < Wo && u >= 0 && u < Wo && v >= 0 && v < Ho) {
            const int X = (yt[2 * v] + xt[2 * u]) >> 5;              // AB_BITS - INTER_BITS
            const int Y = (yt[2 * v + 1] + xt[2 * u + 1]) >> 5;
            const int sx = min(max(X >> 5, -32768), 32767), fx = X & 31;
            const int sy = min(max(Y >> 5, -32768), 32767), fy = Y & 31;
            const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
            // neighbour (p, q) of the intermediate (pre-translated) W x H image: inside it AND its source pixel (p - pre_dx, q - pre_dy) inside
            const int c0 = sx - gg.pre_dx;
            const bool col0 = sx >= 0 && sx < W && c0 >= 0 && c0 < W;
            const bool col1 = sx + 1 >= 0 && sx + 1 < W && c0 + 1 >= 0 && c0 + 1 < W;
            unsigned s[4];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int qq = sy + r, r0 = qq - gg.pre_dy;
                const bool row = qq >= 0 && qq < H && r0 >= 0 && r0 < H;
                const long long off = ((long long)r0 * W + c0) * C;
                load_pair<C>(src, off, total - src_off, row && col0, row && col1, bg, s[2 * r], s[2 * r + 1]);
            }
            out = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int sh = 8 * c;
                const int sum = (int)((s[0] >> sh) & 255) * w00 + (int)((s[1] >> sh) & 255) * w01 + (int)((s[2] >> sh) & 255) * w10 +
                                (int)((s[3] >> sh) & 255) * w11;
                const int val = min(max((sum + (1 << 14)) >> 15, 0), 255);
                out |= (unsigned)val << sh;
            }
        }
        px[k] = out;
    }
    unsigned char* dst = y + ((long long)b * Ho + oy) * Wo * C + (long long)ox0 * C;
    if (ox0 + 4 <= Wo && (Wo & 3) == 0) {                       // 4 C bytes at a 4-byte aligned offset: C dword stores
        unsigned char bytes[4 * C];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) bytes[k * C + c] = (unsigned char)(px[k] >> (8 * c));
#pragma unroll
        for (int d = 0; d < C; ++d) {
            const unsigned w = (unsigned)bytes[4 * d] | ((unsigned)bytes[4 * d + 1] << 8) | ((unsigned)bytes[4 * d + 2] << 16) |
                               ((unsigned)bytes[4 * d + 3] << 24);
            reinterpret_cast<unsigned*>(dst)[d] = w;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (ox0 + k >= Wo) break;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[k * C + c] = (unsigned char)(px[k] >> (8 * c));
    }
}

}  // namespace ssdhip

using namespace ssdhip;

extern "C" int ssdhip_image_warp_affine_u8(const void* x, void* y, int B, int H, int W, int Ho, int Wo, int C, const int* geo_dev,
                                           const int* xtab_dev, const int* ytab_dev, const void* background_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !y || !geo_dev || !xtab_dev || !ytab_dev || !background_dev) return SSDHIP_E_BADARG;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || C < 1 || C > 4 || (long long)H * W > 0x7fffffffLL) return SSDHIP_E_BADARG;
    if (((uintptr_t)y & 3) != 0) return SSDHIP_E_BADARG;
    const long long work = (long long)((Wo + 3) / 4) * Ho;
    const long long blocks = (work + 255) / 256;
    if (blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
    const long long total = (long long)B * H * W * C;
    const unsigned char* xs = static_cast<const unsigned char*>(x);
    unsigned char* ys = static_cast<unsigned char*>(y);
    const unsigned char* bg = static_cast<const unsigned char*>(background_dev);
    const dim3 grid((unsigned)blocks, (unsigned)B);
    switch (C) {
        case 1: hipLaunchKernelGGL(warp_affine_u8_kernel<1>, grid, dim3(256), 0, stream, xs, ys, H, W, Ho, Wo, geo_dev, xtab_dev, ytab_dev, bg, total); break;
        case 2: hipLaunchKernelGGL(warp_affine_u8_kernel<2>, grid, dim3(256), 0, stream, xs, ys, H, W, Ho, Wo, geo_dev, xtab_dev, ytab_dev, bg, total); break;
        case 3: hipLaunchKernelGGL(warp_affine_u8_kernel<3>, grid, dim3(256), 0, stream, xs, ys, H, W, Ho, Wo, geo_dev, xtab_dev, ytab_dev, bg, total); break;
        default: hipLaunchKernelGGL(warp_affine_u8_kernel<4>, grid, dim3(256), 0, stream, xs, ys, H, W, Ho, Wo, geo_dev, xtab_dev, ytab_dev, bg, total); break;
    }
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
