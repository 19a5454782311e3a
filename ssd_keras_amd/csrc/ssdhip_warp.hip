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
//
// Two kernels share that pixel (`warp_pixel`) and differ in what the warp reads: the uniform batch above (the chain's own augment_batch),
// and a RAGGED batch -- images of different sizes, every one with its own tables and output size, the geometry recorded in front of the
// warp as index maps (generate()'s composed lists with Translate / Scale, data_generator/_image_ops.StagedGeoImage).  Both are bound by
// memory traffic and byte gathers (one read of the sources, one write of the results, a handful of cached table ints per pixel): no LDS.
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

// One output pixel of the warp: neighbour coordinates and 15-bit weights from the tables, the four neighbours from `src` (a source that
// answers `row_pair(p, q, a, b)`: the packed pixels (p, q) and (p + 1, q) of the image the warp reads), the rounded blend.  Both kernels
// below compute their pixels here.
template <int C, class Src>
__device__ __forceinline__ unsigned warp_pixel(const Src& src, const int* __restrict__ xt, const int* __restrict__ yt, int u, int v) {
    const int X = (yt[2 * v] + xt[2 * u]) >> 5;              // AB_BITS - INTER_BITS
    const int Y = (yt[2 * v + 1] + xt[2 * u + 1]) >> 5;
    const int sx = min(max(X >> 5, -32768), 32767), fx = X & 31;
    const int sy = min(max(Y >> 5, -32768), 32767), fy = Y & 31;
    const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
    unsigned s[4];
#pragma unroll
    for (int r = 0; r < 2; ++r) src.row_pair(sx, sy + r, s[2 * r], s[2 * r + 1]);
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int sh = 8 * c;
        const int sum = (int)((s[0] >> sh) & 255) * w00 + (int)((s[1] >> sh) & 255) * w01 + (int)((s[2] >> sh) & 255) * w10 +
                        (int)((s[3] >> sh) & 255) * w11;
        const int val = min(max((sum + (1 << 14)) >> 15, 0), 255);
        out |= (unsigned)val << sh;
    }
    return out;
}

// four adjacent output pixels (packed, byte k = channel k) to row position ox0 of a Wo-pixel row at dst: C dword stores when the row
// allows it (`dwords`: Wo % 4 == 0 and the image 4-byte aligned), bytes otherwise
template <int C>
__device__ __forceinline__ void store_quad(unsigned char* __restrict__ dst, const unsigned (&px)[4], int ox0, int Wo, bool dwords) {
    if (ox0 + 4 <= Wo && dwords) {
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

// the uniform batch's source: neighbour (p, q) of the intermediate (pre-translated) W x H image is inside it AND its source pixel
// (p - pre_dx, q - pre_dy) is inside; the background otherwise
template <int C>
struct UniformWarpSrc {
    const unsigned char* __restrict__ src;
    long long total;                                         // bytes from src to the end of the batch
    int H, W, pre_dx, pre_dy;
    unsigned bg;
    __device__ __forceinline__ void row_pair(int p, int q, unsigned& a, unsigned& b) const {
        const int c0 = p - pre_dx, r0 = q - pre_dy;
        const bool col0 = p >= 0 && p < W && c0 >= 0 && c0 < W;
        const bool col1 = p + 1 >= 0 && p + 1 < W && c0 + 1 >= 0 && c0 + 1 < W;
        const bool row = q >= 0 && q < H && r0 >= 0 && r0 < H;
        const long long off = ((long long)r0 * W + c0) * C;
        load_pair<C>(src, off, total, row && col0, row && col1, bg, a, b);
    }
};

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
    const long long src_off = (long long)b * H * W * C;
    const UniformWarpSrc<C> src = {x + src_off, total - src_off, H, W, gg.pre_dx, gg.pre_dy, bg};
    const int* xt = xtab + (long long)b * Wo * 2;
    const int* yt = ytab + (long long)b * Ho * 2;

    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ox = ox0 + k;
        const int x1 = gg.flip ? Wo - 1 - ox : ox;
        const int u = x1 - gg.post_dx, v = oy - gg.post_dy;
        px[k] = (ox < Wo && u >= 0 && u < Wo && v >= 0 && v < Ho) ? warp_pixel<C>(src, xt, yt, u, v) : bg;
    }
    store_quad<C>(y + ((long long)b * Ho + oy) * Wo * C + (long long)ox0 * C, px, ox0, Wo, (Wo & 3) == 0);
}

// ---- ragged batches: every image its own size, its own tables, and the index maps of the geometry recorded in front of the warp --------
// The warp of image b reads a VIRTUAL ha x wa image: position (q, p) shows source pixel (ys[q], xs[p]) of image b (read through the
// ragged table, C = 1 replicated, C = 4 alpha dropped: ConvertTo3Channels, as the ragged gather reads), the padding colour where
// either map says -1, black where either says -2.  A neighbour outside ha x wa reads the warp's border colour -- and so does anything
// that would address memory outside image b (a map entry below -2 or past the image, a table row that does not lie inside the buffer):
// nothing is clamped.
struct RaggedWarpSrc {
    const unsigned char* __restrict__ x;
    long long total, off;                                    // bytes in x; image b's first byte
    int H, W, C;                                             // H = W = 0: the table's row is not inside the buffer
    const int* __restrict__ xs;
    const int* __restrict__ ys;
    int wa, ha;
    unsigned border, padding;

    enum { OUTSIDE = -3 };
    __device__ __forceinline__ static int entry(const int* __restrict__ map, int n, int k, int limit) {
        if (k < 0 || k >= n) return OUTSIDE;
        const int e = map[k];
        return (e < -2 || e >= limit) ? (int)OUTSIDE : e;
    }
    __device__ __forceinline__ unsigned pixel(int ry, int cx) const {
        if (ry == OUTSIDE || cx == OUTSIDE) return border;
        if (ry == -2 || cx == -2) return 0u;
        if (ry == -1 || cx == -1) return padding;
        const unsigned char* p = x + off + ((long long)ry * W + cx) * C;
        if (C == 1) return (unsigned)p[0] * 0x010101u;
        return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    }
    __device__ __forceinline__ void row_pair(int p, int q, unsigned& a, unsigned& b) const {
        const int ry = entry(ys, ha, q, H);
        const int c0 = entry(xs, wa, p, W), c1 = entry(xs, wa, p + 1, W);
        if (C == 3 && ry >= 0 && c0 >= 0 && c1 == c0 + 1) {             // two real pixels in adjacent columns: one 8-byte load
            const long long o = off + ((long long)ry * W + c0) * 3;
            if (o + 8 <= total) {
                const uint64_t v = *reinterpret_cast<const u64_unaligned*>(x + o);
                a = (unsigned)(v & 0xffffffull);
                b = (unsigned)((v >> 24) & 0xffffffull);
                return;
            }
        }
        a = pixel(ry, c0);
        b = pixel(ry, c1);
    }
};

// meta [B][8] int32: offsets into `tabs` of xtab (Wo x 2), ytab (Ho x 2), xs (wa), ys (ha); wa, ha; border and padding colour (R | G << 8
// | B << 16).  dst_table [B][4] int64: byte offset into y (a multiple of 4 for the dword stores), Ho, Wo, 3.
__global__ __launch_bounds__(256) void warp_affine_ragged_u8_kernel(const unsigned char* __restrict__ x, long long x_bytes,
                                                                    const long long* __restrict__ src_table, unsigned char* __restrict__ y,
                                                                    long long y_bytes, const long long* __restrict__ dst_table,
                                                                    const int* __restrict__ tabs, long long n_tabs,
                                                                    const int* __restrict__ meta) {
    const int b = blockIdx.y;
    const long long* dt = dst_table + 4 * (long long)b;
    const long long dst_off = dt[0], Ho_ = dt[1], Wo_ = dt[2];
    if (dst_off < 0 || Ho_ <= 0 || Wo_ <= 0 || Ho_ > 0x7fffffffLL || Wo_ > 0x7fffffffLL || dt[3] != 3 ||
        Ho_ * Wo_ * 3 > y_bytes - dst_off)
        return;                                              // not a row of this buffer (the launcher's caller checks it on the host)
    const int Ho = (int)Ho_, Wo = (int)Wo_;
    const int quads = (Wo + 3) >> 2;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)quads * Ho) return;
    const int* m = meta + 8 * (long long)b;
    const int wa = m[4], ha = m[5];
    const long long o_xt = m[0], o_yt = m[1], o_xs = m[2], o_ys = m[3];
    if (wa < 0 || ha < 0 || o_xt < 0 || o_yt < 0 || o_xs < 0 || o_ys < 0 || o_xt + 2LL * Wo > n_tabs || o_yt + 2LL * Ho > n_tabs ||
        o_xs + wa > n_tabs || o_ys + ha > n_tabs)
        return;
    const long long* st = src_table + 4 * (long long)b;
    const long long off = st[0], H = st[1], W = st[2], C = st[3];
    const bool inside = off >= 0 && H > 0 && W > 0 && H <= 0x7fffffffLL && W <= 0x7fffffffLL && (C == 1 || C == 3 || C == 4) &&
                        H * W * C <= x_bytes - off;
    const RaggedWarpSrc src = {x, x_bytes, off, inside ? (int)H : 0, inside ? (int)W : 0, (int)C, tabs + o_xs, tabs + o_ys, wa, ha,
                               (unsigned)m[6] & 0xffffffu, (unsigned)m[7] & 0xffffffu};
    const int oy = (int)(q / quads);
    const int ox0 = (int)(q - (long long)oy * quads) * 4;
    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = (ox0 + k < Wo) ? warp_pixel<3>(src, tabs + o_xt, tabs + o_yt, ox0 + k, oy) : 0u;
    store_quad<3>(y + dst_off + ((long long)oy * Wo + ox0) * 3, px, ox0, Wo, (Wo & 3) == 0 && (dst_off & 3) == 0);
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

// cv2.warpAffine for a ragged batch in one launch (the contract is in include/ssdhip.h): grid (the largest image's quads / 256, B),
// threads past their image's work return.
extern "C" int ssdhip_image_warp_affine_ragged_u8(const void* x, long long x_bytes, const long long* src_table_dev, void* y, long long y_bytes,
                                                  const long long* dst_table_dev, int B, long long max_work, const int* tabs_dev,
                                                  long long n_tabs, const int* meta_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !src_table_dev || !y || !dst_table_dev || !tabs_dev || !meta_dev) return SSDHIP_E_BADARG;
    if (B <= 0 || B > 65535 || x_bytes <= 0 || y_bytes <= 0 || n_tabs <= 0 || n_tabs > 0x7fffffffLL || max_work <= 0) return SSDHIP_E_BADARG;
    if (((uintptr_t)y & 3) != 0) return SSDHIP_E_BADARG;
    const long long blocks = (max_work + 255) / 256;
    if (blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(warp_affine_ragged_u8_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, stream,
                       static_cast<const unsigned char*>(x), x_bytes, src_table_dev, static_cast<unsigned char*>(y), y_bytes, dst_table_dev,
                       tabs_dev, n_tabs, meta_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
