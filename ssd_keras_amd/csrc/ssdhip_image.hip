// ssdhip_image.hip -- the image half of the reference's training-time augmentation on gfx950 (MI355X): SURVEY 8f row 4.
//
// The reference distorts one NumPy image at a time on the host through OpenCV (data_generator/object_detection_2d_photometric_ops.py
// :23-480, object_detection_2d_geometric_ops.py:27-148, the chain data_augmentation_chain_original_ssd.py:146-280); a batch-32 step of
// the detector takes 2.3 ms here, so the input pipeline has to live where the images are.  Three kernels:
//   * pixel_program_kernel   every POINTWISE operation of the photometric ops as a per-image program of up to 16 (op, argument) steps
//                            run by one thread per pixel: dtype conversions (the reference's uint8 <-> float32 round trips with
//                            their roundings), brightness / contrast / saturation / hue in NumPy's arithmetic for the array's
//                            dtype (float32 ops for float32 images, float64 for uint8 ones, truncating in-place stores), 8-bit and
//                            float32 RGB <-> HSV, grey, channel permutations.  One launch distorts a whole batch, each image with
//                            its own program (the random draws stay on the host, in the reference's order);
//   * resize_cv_kernel / resize_gather_cv_kernel   cv2.resize with OpenCV's own 8-bit arithmetic, from a plan of source indices
//                            and weights per output column / row (one plan for the batch, or one per image with the augmentation
//                            chain's expansion / crop / flip composed in; resize_gather_turn_cv_kernel: the same for plans that
//                            hold a rotation by quarter turns -- a transposed bit per image swaps the source address);
//   * hist_u8_kernel / lut_u8_kernel   cv2.equalizeHist (histogram on the device, the 256-entry table on the host) and cv2.LUT, one image
//                            at a time; for a batch both are steps of the programs: OP_LUT reads one of four tables per image,
//                            program_hist_u8_kernel counts a channel of the state a program reaches at a given step and
//                            equalize_tables_kernel turns the histograms into tables, one wave per image -- no host round trip.
// Arithmetic is written operation by operation (-ffp-contract=off): bit-identical to the NumPy restatement in oracle/np_image.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_math.h"

namespace ssdhip {

enum { IMG_U8 = 0, IMG_F32 = 1, IMG_F64 = 2 };
enum { OP_END = 0, OP_TO_F32 = 1, OP_TO_U8 = 2, OP_BRIGHTNESS = 3, OP_CONTRAST = 4, OP_SATURATION = 5, OP_HUE = 6, OP_RGB2HSV = 7,
       OP_HSV2RGB = 8, OP_RGB2GRAY = 9, OP_SWAP = 10, OP_LUT = 11 };
constexpr int IMG_PROG = 16;
constexpr int IMG_LUT_SLOTS = 4;                             // tables per image: luts [n_images][IMG_LUT_SLOTS][256] uint8

__device__ __forceinline__ double img_clip255(double v) { return v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v); }
__device__ __forceinline__ float img_clip255f(float v) { return v < 0.f ? 0.f : (v > 255.f ? 255.f : v); }
// np.remainder (the sign of the divisor), float32 / float64
__device__ __forceinline__ float img_modf(float a, float b) {
    float m = fmodf(a, b);
    if (m != 0.f) { if ((b < 0.f) != (m < 0.f)) m += b; } else m = copysignf(0.f, b);
    return m;
}
__device__ __forceinline__ double img_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) { if ((b < 0.0) != (m < 0.0)) m += b; } else m = copysign(0.0, b);
    return m;
}
// value stored into a uint8 array by `a[..] = float_expression`: C truncation (the callers keep it inside [0, 255])
__device__ __forceinline__ double img_trunc_u8(double v) { return (double)(unsigned char)(int)v; }

__device__ __forceinline__ int img_div_table(int numerator_shifted, int i, int six) {      // saturate_cast<int>(num / (six * i)): nearest, ties to even
    if (i == 0) return 0;
    const int den = six * i;
    int q = numerator_shifted / den;
    const int r = numerator_shifted - q * den;
    if (2 * r > den || (2 * r == den && (q & 1))) ++q;
    return q;
}

// sdiv / hdiv: OpenCV's two 256-entry division tables (saturate_cast<int>((255 << 12) / v), ((180 << 12) / (6 diff))) in LDS, or null:
// the entries computed on the spot (two integer divisions per pixel -- what the first version did for every pixel)
__device__ __forceinline__ void img_rgb2hsv_u8(double (&c)[3], const int* sdiv = nullptr, const int* hdiv = nullptr) {
    const int r = (int)c[0], g = (int)c[1], b = (int)c[2];
    const int v = max(max(r, g), b), vmin = min(min(r, g), b), diff = v - vmin;
    const int s = (diff * (sdiv ? sdiv[v] : img_div_table(255 << 12, v, 1)) + (1 << 11)) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * (hdiv ? hdiv[diff] : img_div_table(180 << 12, diff, 6)) + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    c[0] = (double)min(max(h, 0), 255); c[1] = (double)s; c[2] = (double)v;
}

__device__ __forceinline__ void img_hsv2rgb_float(float h, float s, float v, float hscale, float (&rgb)[3]) {
    if (s == 0.f) { rgb[0] = rgb[1] = rgb[2] = v; return; }
    h = h * hscale;
    if (h < 0.f) h = h + 6.f;
    if (h >= 6.f) h = h - 6.f;
    int sector = (int)floorf(h);
    h = h - (float)sector;
    if (sector < 0 || sector >= 6) { sector = 0; h = 0.f; }
    float tab[4];
    tab[0] = v;
    tab[1] = v * (1.f - s);
    tab[2] = v * (1.f - s * h);
    tab[3] = v * (1.f - s * (1.f - h));
    const int pick[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};      // (b, g, r)
    rgb[2] = tab[pick[sector][0]]; rgb[1] = tab[pick[sector][1]]; rgb[0] = tab[pick[sector][2]];
}

__device__ __forceinline__ void img_rgb2hsv_f32(double (&c)[3]) {
    const float r = (float)c[0], g = (float)c[1], b = (float)c[2];
    const float eps = 1.1920928955078125e-07f;
    const float v = fmaxf(fmaxf(r, g), b), vmin = fminf(fminf(r, g), b);
    const float diff = v - vmin;
    const float s = diff / (fabsf(v) + eps);
    const float d = 60.f / (diff + eps);
    float h = v == r ? (g - b) * d : (v == g ? (b - r) * d + 120.f : (r - g) * d + 240.f);
    if (h < 0.f) h = h + 360.f;
    c[0] = (double)h; c[1] = (double)s; c[2] = (double)v;
}

// One program step on N pixels (the same step for all of them: a program is per image).  `tag` = the dtype the reference's array has at
// this point of the chain; arithmetic per dtype as NumPy / OpenCV do it (see the file header).  `lut`: the image's IMG_LUT_SLOTS tables
// (in LDS or in global memory), or null: OP_LUT then leaves the pixel alone, as it does on a float state -- ssdhip_image_program_check
// refuses both while the program is still on the host.
template <int N>
__device__ __forceinline__ void img_apply(double (&px)[N][3], int& tag, const int o, const double a, const int* sdiv, const int* hdiv,
                                          const unsigned char* lut = nullptr) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        double (&c)[3] = px[n];
        if (o == OP_TO_F32) {
            if (tag == IMG_F64) { c[0] = (double)(float)c[0]; c[1] = (double)(float)c[1]; c[2] = (double)(float)c[2]; }
        } else if (o == OP_TO_U8) {                                  // np.round(image, 0).astype(uint8)
#pragma unroll
            for (int q = 0; q < 3; ++q) c[q] = img_clip255(tag == IMG_F32 ? (double)rintf((float)c[q]) : rint(c[q]));
        } else if (o == OP_BRIGHTNESS) {                             // np.clip(image + delta, 0, 255)
            if (tag == IMG_F32) {
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = (double)img_clip255f((float)c[q] + (float)a);
            } else {
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = img_clip255(c[q] + a);
            }
        } else if (o == OP_CONTRAST) {                               // np.clip(127.5 + factor * (image - 127.5), 0, 255)
            if (tag == IMG_F32) {
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = (double)img_clip255f(127.5f + (float)a * ((float)c[q] - 127.5f));
            } else {
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = img_clip255(127.5 + a * (c[q] - 127.5));
            }
        } else if (o == OP_SATURATION) {                             // image[:, :, 1] = np.clip(image[:, :, 1] * factor, 0, 255)
            if (tag == IMG_F32) c[1] = (double)img_clip255f((float)c[1] * (float)a);
            else if (tag == IMG_U8) c[1] = img_trunc_u8(img_clip255(c[1] * a));
            else c[1] = img_clip255(c[1] * a);
        } else if (o == OP_HUE) {                                    // image[:, :, 0] = (image[:, :, 0] + delta) % 180.0
            if (tag == IMG_F32) c[0] = (double)img_modf((float)c[0] + (float)a, 180.f);
            else if (tag == IMG_U8) c[0] = img_trunc_u8(img_mod(c[0] + a, 180.0));
            else c[0] = img_mod(c[0] + a, 180.0);
        } else if (o == OP_RGB2HSV) {
            if (tag == IMG_U8) img_rgb2hsv_u8(c, sdiv, hdiv);
            else img_rgb2hsv_f32(c);
        } else if (o == OP_HSV2RGB) {
            float rgb[3];
            if (tag == IMG_U8) {
                img_hsv2rgb_float((float)c[0], (float)c[1] * (float)(1.0 / 255.0), (float)c[2] * (float)(1.0 / 255.0), (float)(6.0 / 180.0), rgb);
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = (double)img_clip255f(rintf(rgb[q] * 255.f));
            } else {
                img_hsv2rgb_float((float)c[0], (float)c[1], (float)c[2], (float)(6.0 / 360.0), rgb);
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = (double)rgb[q];
            }
        } else if (o == OP_RGB2GRAY) {
            double gr;
            if (tag == IMG_U8) {
                gr = (double)(((int)c[0] * 4899 + (int)c[1] * 9617 + (int)c[2] * 1868 + (1 << 13)) >> 14);
            } else {
                const float t = (float)c[0] * 0.299f + (float)c[1] * 0.587f;
                gr = (double)(t + (float)c[2] * 0.114f);
            }
            c[0] = c[1] = c[2] = gr;
        } else if (o == OP_SWAP) {                                   // image[:, :, order], order packed as o0 + 4 o1 + 16 o2
            const int code = (int)a;
            const double t0 = c[code & 3], t1 = c[(code >> 2) & 3], t2 = c[(code >> 4) & 3];
            c[0] = t0; c[1] = t1; c[2] = t2;
        } else if (o == OP_LUT) {                                    // cv2.LUT: v = table[v]; argument = slot + 4 * channel mask
            if (lut && tag == IMG_U8) {
                const int code = (int)a;
                const unsigned char* t = lut + (code & (IMG_LUT_SLOTS - 1)) * 256;
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if ((code >> (2 + q)) & 1) c[q] = (double)t[(int)c[q] & 255];
            }
        }
    }
    // the dtype after the step (the same for every pixel)
    if (o == OP_TO_F32) tag = IMG_F32;
    else if (o == OP_TO_U8) tag = IMG_U8;
    else if ((o == OP_BRIGHTNESS || o == OP_CONTRAST) && tag != IMG_F32) tag = IMG_F64;
}

// x: [n_images][pixels][3] uint8, float32 or float64; y: uint8 / float32 / float64 as out_tag says; ops / args: [n_images][IMG_PROG].
__global__ __launch_bounds__(256) void pixel_program_kernel(const void* __restrict__ x, int in_tag, void* __restrict__ y, int out_tag,
                                                            long long pixels, const int* __restrict__ ops, const double* __restrict__ args,
                                                            const unsigned char* __restrict__ luts) {
    const int img = blockIdx.y;
    const int* op = ops + (size_t)img * IMG_PROG;
    const double* arg = args + (size_t)img * IMG_PROG;
    const unsigned char* lut = luts ? luts + (size_t)img * IMG_LUT_SLOTS * 256 : nullptr;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
        const size_t e = ((size_t)img * pixels + p) * 3;
        double c[3];
        int tag = in_tag;
        if (in_tag == IMG_U8) {
            const unsigned char* s = static_cast<const unsigned char*>(x) + e;
            c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
        } else if (in_tag == IMG_F32) {
            const float* s = static_cast<const float*>(x) + e;
            c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
        } else {
            const double* s = static_cast<const double*>(x) + e;
            c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
        }
        double px[1][3] = {{c[0], c[1], c[2]}};
        for (int k = 0; k < IMG_PROG; ++k) {
            const int o = op[k];
            if (o == OP_END) break;
            img_apply<1>(px, tag, o, arg[k], nullptr, nullptr, lut);
        }
        c[0] = px[0][0]; c[1] = px[0][1]; c[2] = px[0][2];
        if (out_tag == IMG_U8) {
            unsigned char* d = static_cast<unsigned char*>(y) + e;
            d[0] = (unsigned char)c[0]; d[1] = (unsigned char)c[1]; d[2] = (unsigned char)c[2];
        } else if (out_tag == IMG_F32) {
            float* d = static_cast<float*>(y) + e;
            d[0] = (float)c[0]; d[1] = (float)c[1]; d[2] = (float)c[2];
        } else {
            double* d = static_cast<double*>(y) + e;
            d[0] = c[0]; d[1] = c[1]; d[2] = c[2];
        }
    }
}

// How a batch's images are laid out: image `img` starts `offset(img)` bytes into the buffer and has `count(img)` pixels.  Uniform: the
// (B, H, W, 3) tensor.  Ragged: B images of different sizes in one buffer, table [B][4] int64 = byte offset, H, W, C (the offsets 256-byte
// aligned by the host, so every image starts on a dword).
struct UniformImages {
    long long pixels;
    __device__ __forceinline__ long long offset(int img) const { return (long long)img * pixels * 3; }
    __device__ __forceinline__ long long count(int) const { return pixels; }
};
struct RaggedImages {
    const long long* table;
    __device__ __forceinline__ long long offset(int img) const { return table[(size_t)img * 4]; }
    __device__ __forceinline__ long long count(int img) const { return table[(size_t)img * 4 + 1] * table[(size_t)img * 4 + 2]; }
};

// The uint8 -> uint8 form (the photometric distortions of a whole batch): FOUR pixels = 12 bytes = three dwords per thread and trip, so
// a wave moves 768 contiguous bytes per load / store instruction instead of 64 single bytes at a 3-byte stride; every program step is
// decoded once for the four pixels; OpenCV's two 8-bit HSV division tables sit in LDS (built once per workgroup) instead of two integer
// divisions per pixel.  Same arithmetic, same results as pixel_program_kernel.  The last count % 4 pixels of an image (ragged batches
// only: the uniform form is launched for pixels % 4 == 0) take one work item each, byte by byte.  `luts` (or null): the image's four
// tables come into LDS once per workgroup, one dword per thread.
template <class Imgs>
__global__ __launch_bounds__(256) void pixel_program_u8x4_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, Imgs imgs,
                                                                 const int* __restrict__ ops, const double* __restrict__ args,
                                                                 const unsigned char* __restrict__ luts) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ unsigned int slut[IMG_LUT_SLOTS * 64];
    const int img = blockIdx.y;
    sdiv[threadIdx.x] = img_div_table(255 << 12, (int)threadIdx.x, 1);
    hdiv[threadIdx.x] = img_div_table(180 << 12, (int)threadIdx.x, 6);
    if (luts) slut[threadIdx.x] = reinterpret_cast<const unsigned int*>(luts)[(size_t)img * IMG_LUT_SLOTS * 64 + threadIdx.x];
    __syncthreads();
    const unsigned char* lut = luts ? reinterpret_cast<const unsigned char*>(slut) : nullptr;
    const int* op = ops + (size_t)img * IMG_PROG;
    const double* arg = args + (size_t)img * IMG_PROG;
    const long long pixels = imgs.count(img), off = imgs.offset(img);
    const unsigned int* xw = reinterpret_cast<const unsigned int*>(x + off);
    unsigned int* yw = reinterpret_cast<unsigned int*>(y + off);
    const long long groups = pixels / 4, items = groups + (pixels - groups * 4);
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < items; g += (long long)gridDim.x * 256) {
        if (g >= groups) {                                               // the tail: one pixel
            const size_t e = (size_t)(groups * 4 + (g - groups)) * 3;
            double px[1][3] = {{(double)x[off + e], (double)x[off + e + 1], (double)x[off + e + 2]}};
            int tag = IMG_U8;
            for (int k = 0; k < IMG_PROG; ++k) {
                const int o = op[k];
                if (o == OP_END) break;
                img_apply<1>(px, tag, o, arg[k], sdiv, hdiv, lut);
            }
            y[off + e] = (unsigned char)px[0][0]; y[off + e + 1] = (unsigned char)px[0][1]; y[off + e + 2] = (unsigned char)px[0][2];
            continue;
        }
        const size_t e = (size_t)g * 3;                                  // dword index of the group's 12 bytes
        const unsigned int w0 = xw[e], w1 = xw[e + 1], w2 = xw[e + 2];
        double px[4][3];
        px[0][0] = w0 & 255u; px[0][1] = (w0 >> 8) & 255u; px[0][2] = (w0 >> 16) & 255u;
        px[1][0] = w0 >> 24; px[1][1] = w1 & 255u; px[1][2] = (w1 >> 8) & 255u;
        px[2][0] = (w1 >> 16) & 255u; px[2][1] = w1 >> 24; px[2][2] = w2 & 255u;
        px[3][0] = (w2 >> 8) & 255u; px[3][1] = (w2 >> 16) & 255u; px[3][2] = w2 >> 24;
        int tag = IMG_U8;
        for (int k = 0; k < IMG_PROG; ++k) {
            const int o = op[k];
            if (o == OP_END) break;
            img_apply<4>(px, tag, o, arg[k], sdiv, hdiv, lut);
        }
        unsigned int b[12];
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int q = 0; q < 3; ++q) b[n * 3 + q] = (unsigned int)(unsigned char)px[n][q];
        yw[e] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        yw[e + 1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        yw[e + 2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// cv2.resize on 8-bit images with OpenCV's OWN arithmetic (round 6; imgproc/resize.cpp, the C++ reference paths).  The host (data_generator/_image_ops.py
// resize_plan) or the device (csrc/ssdhip_augment.hip) builds the plan: `kind`, tap indices, and the tables as float64 values that hold
// 11-bit fixed-point shorts / float32 area weights / ones exactly.  Per output value, rows j outer, columns k inner:
//   COPY / NEAREST   the single tap
//   LINEAR           S_j = p[j][0] a0 + p[j][1] a1 (int32);  uchar((((b0 (S_0 >> 4)) >> 16) + ((b1 (S_1 >> 4)) >> 16) + 2) >> 2)
//                    (VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>: the two-stage form of its mulhi SIMD twin)
//   KERNEL           cubic / Lanczos-4: S_j = sum_k p a_k, saturate((sum_j S_j b_j + (1 << 21)) >> 22), int32 (wrapping) arithmetic
//   AREA             ResizeArea: buf_j = sum_k float(p) alpha_k, total = sum_j beta_j buf_j, all float32 in table order, cvRound, saturate
//   AREA_FAST / 2    ResizeAreaFast: the block's integer sum; saturate(cvRound(float(sum) * (1.f / area))); 2 x 2: (sum + 2) >> 2
// Unused taps of a padded row carry weight 0 and a valid index (a float32 sum is unchanged by + p * 0.f).
// ---------------------------------------------------------------------------------------------------------------------------------------
enum { CV_NEAREST = 0, CV_LINEAR = 1, CV_KERNEL = 2, CV_AREA = 3, CV_AREA_FAST = 4, CV_AREA_FAST2 = 5, CV_COPY = 6 };

template <typename Px>
__device__ __forceinline__ unsigned char cv_resample(const int kind, const int area, const int nx, const int ny, const double* __restrict__ wx,
                                                     const double* __restrict__ wy, Px px) {
    if (kind == CV_NEAREST || kind == CV_COPY) return (unsigned char)px(0, 0);
    if (kind == CV_LINEAR) {
        const int a0 = (int)wx[0], a1 = (int)wx[1], b0 = (int)wy[0], b1 = (int)wy[1];
        const int s0 = px(0, 0) * a0 + px(0, 1) * a1, s1 = px(1, 0) * a0 + px(1, 1) * a1;
        return (unsigned char)((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2);
    }
    if (kind == CV_KERNEL) {
        unsigned int acc = 0u;                                        // unsigned: the wrap-around of the reference's int arithmetic, defined
        for (int j = 0; j < ny; ++j) {
            unsigned int row = 0u;
            for (int k = 0; k < nx; ++k) row += (unsigned int)(px(j, k) * (int)wx[k]);
            acc += row * (unsigned int)(int)wy[j];
        }
        const int v = ((int)(acc + (1u << 21))) >> 22;
        return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
    if (kind == CV_AREA) {
        float total = 0.f;
        for (int j = 0; j < ny; ++j) {
            float buf = 0.f;
            for (int k = 0; k < nx; ++k) buf = buf + (float)px(j, k) * (float)wx[k];
            const float term = (float)wy[j] * buf;
            total = j == 0 ? term : total + term;
        }
        const float r = rintf(total);
        return (unsigned char)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
    }
    int sum = 0;
    for (int j = 0; j < ny; ++j)
        for (int k = 0; k < nx; ++k) sum += px(j, k);
    if (kind == CV_AREA_FAST2) return (unsigned char)((sum + 2) >> 2);
    const float r = rintf((float)sum * (1.f / (float)area));
    return (unsigned char)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

// one plan for the whole batch: grid (blocks over Wo C, Ho, B); ix / wx [Wo][nx], iy / wy [Ho][ny]
__global__ __launch_bounds__(256) void resize_cv_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W,
                                                        int Ho, int Wo, int C, int kind, int area, const int* __restrict__ ix,
                                                        const double* __restrict__ wx, int nx, const int* __restrict__ iy,
                                                        const double* __restrict__ wy, int ny) {
    const int v = (int)blockIdx.x * 256 + (int)threadIdx.x, yo = (int)blockIdx.y, b = (int)blockIdx.z;
    if (v >= Wo * C) return;
    const int xo = v / C, ch = v - xo * C;
    const unsigned char* src = x + (size_t)b * H * W * C;
    const int* ixr = ix + (size_t)xo * nx;
    const int* iyr = iy + (size_t)yo * ny;
    auto px = [&](int j, int k) -> int { return (int)src[((size_t)iyr[j] * W + ixr[k]) * C + ch]; };
    y[((size_t)b * Ho + yo) * Wo * C + v] = cv_resample(kind, area, nx, ny, wx + (size_t)xo * nx, wy + (size_t)yo * ny, px);
}

// Where the gather reads image b's channel ch: `at(sy, sx)` = the source value at row sy, column sx.  Uniform: the (B, H, W, C) tensor.
// Ragged: the table [B][4] of RaggedImages, output channel ch read from source channel ch (C = 3, 4: alpha never read) or 0 (C = 1, grey
// replicated) -- ConvertTo3Channels folded into the read; indices clamped into the image (a plan built for other sizes cannot leave it).
struct UniformGatherSrc {
    const unsigned char* x;
    int H, W, C;
    struct View {
        const unsigned char* p;
        int W, C;
        __device__ __forceinline__ int at(int sy, int sx) const { return (int)p[((size_t)sy * W + sx) * C]; }
    };
    __device__ __forceinline__ View view(int b, int ch) const { return View{x + (size_t)b * H * W * C + ch, W, C}; }
    __device__ __forceinline__ int height(int) const { return H; }
    __device__ __forceinline__ int width(int) const { return W; }
};
struct RaggedGatherSrc {
    const unsigned char* x;
    const long long* table;
    struct View {
        const unsigned char* p;
        int H, W, C;
        __device__ __forceinline__ int at(int sy, int sx) const {
            sy = sy < H ? sy : H - 1; sx = sx < W ? sx : W - 1;
            return (int)p[((size_t)sy * W + sx) * C];
        }
    };
    __device__ __forceinline__ View view(int b, int ch) const {
        const long long* t = table + (size_t)b * 4;
        const int c = (int)t[3];
        return View{x + t[0] + (c == 1 ? 0 : ch), (int)t[1], (int)t[2], c};
    }
    __device__ __forceinline__ int height(int b) const { return (int)table[(size_t)b * 4 + 1]; }
    __device__ __forceinline__ int width(int b) const { return (int)table[(size_t)b * 4 + 2]; }
};

// every image its own plan (the augmentation chain's gather launch): plan [B][4] = kind, area, taps per column, taps per row (<= nx, ny =
// the tables' strides); ix / wx [B][Wo][nx], iy / wy [B][Ho][ny]; index -1 = the expansion canvas -> background [B][C]
template <class Src>
__global__ __launch_bounds__(256) void resize_gather_cv_kernel(Src src, unsigned char* __restrict__ y, int Ho, int Wo, int C,
                                                               const int* __restrict__ plan, const int* __restrict__ ix,
                                                               const double* __restrict__ wx, int nx, const int* __restrict__ iy,
                                                               const double* __restrict__ wy, int ny,
                                                               const unsigned char* __restrict__ background) {
    const int v = (int)blockIdx.x * 256 + (int)threadIdx.x, yo = (int)blockIdx.y, b = (int)blockIdx.z;
    if (v >= Wo * C) return;
    const int xo = v / C, ch = v - xo * C;
    const int kind = plan[b * 4], area = plan[b * 4 + 1], tx = plan[b * 4 + 2], ty = plan[b * 4 + 3];
    const int bg = (int)background[b * C + ch];
    const int* ixb = ix + ((size_t)b * Wo + xo) * nx;
    const int* iyb = iy + ((size_t)b * Ho + yo) * ny;
    const typename Src::View img = src.view(b, ch);
    auto px = [&](int j, int k) -> int {
        const int sy = iyb[j], sx = ixb[k];
        return (sy < 0 || sx < 0) ? bg : img.at(sy, sx);
    };
    y[((size_t)b * Ho + yo) * Wo * C + v] = cv_resample(kind, area, tx < nx ? tx : nx, ty < ny ? ty : ny, wx + ((size_t)b * Wo + xo) * nx,
                                                        wy + ((size_t)b * Ho + yo) * ny, px);
}

// The gather for plans that hold a rotation by quarter turns (ssdhip_sat_augment_plans): transposed [B] = 1 -> image b's ROW table (iy)
// addresses source columns and its column table (ix) source rows, so the source address is swapped; index -1 = background [B][C] (the
// patch's padding), -2 = 0 (what the rotation's warpAffine leaves outside the source), -1 in either table wins.  Indices are clamped into
// the image.  Same arithmetic (cv_resample), grid and tables as resize_gather_cv_kernel.
template <class Src>
__global__ __launch_bounds__(256) void resize_gather_turn_cv_kernel(Src src, unsigned char* __restrict__ y, int Ho, int Wo, int C,
                                                                    const int* __restrict__ plan, const int* __restrict__ ix,
                                                                    const double* __restrict__ wx, int nx, const int* __restrict__ iy,
                                                                    const double* __restrict__ wy, int ny,
                                                                    const int* __restrict__ transposed,
                                                                    const unsigned char* __restrict__ background) {
    const int v = (int)blockIdx.x * 256 + (int)threadIdx.x, yo = (int)blockIdx.y, b = (int)blockIdx.z;
    if (v >= Wo * C) return;
    const int xo = v / C, ch = v - xo * C;
    const int kind = plan[b * 4], area = plan[b * 4 + 1], tx = plan[b * 4 + 2], ty = plan[b * 4 + 3];
    const int bg = (int)background[b * C + ch];
    const bool turned = transposed[b] != 0;
    const int* ixb = ix + ((size_t)b * Wo + xo) * nx;
    const int* iyb = iy + ((size_t)b * Ho + yo) * ny;
    const typename Src::View img = src.view(b, ch);
    const int H = src.height(b), W = src.width(b);
    auto px = [&](int j, int k) -> int {
        const int a = iyb[j], c = ixb[k];
        if (a == -1 || c == -1) return bg;
        if (a < 0 || c < 0) return 0;
        int sy = turned ? c : a, sx = turned ? a : c;
        sy = sy < H ? sy : H - 1; sx = sx < W ? sx : W - 1;
        return img.at(sy, sx);
    };
    y[((size_t)b * Ho + yo) * Wo * C + v] = cv_resample(kind, area, tx < nx ? tx : nx, ty < ny ? ty : ny, wx + ((size_t)b * Wo + xo) * nx,
                                                        wy + ((size_t)b * Ho + yo) * ny, px);
}

__global__ __launch_bounds__(256) void hist_u8_kernel(const unsigned char* __restrict__ x, long long n_pixels, int C, int channel,
                                                      unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n_pixels; p += (long long)gridDim.x * 256)
        atomicAdd(&h[x[(size_t)p * C + channel]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// y = x with table[] applied to the channels whose bit is set in channel_mask
__global__ __launch_bounds__(256) void lut_u8_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, long long n_values,
                                                     int C, int channel_mask, const unsigned char* __restrict__ table) {
    __shared__ unsigned char t[256];
    t[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_values; i += (long long)gridDim.x * 256) {
        const unsigned char v = x[i];
        y[i] = ((channel_mask >> (int)(i % C)) & 1) ? t[v] : v;
    }
}

// cv2.equalizeHist's first half INSIDE a program: image i runs its program up to, not including, step stop[i] and channel channel[i] of
// the uint8 state it reaches is counted into hist[i][256]; stop[i] < 0 = the image takes no part (its row keeps the zeros of the export's
// zero-fill).  Nothing else is written: the half-distorted image never exists in memory.  Pixels are read as pixel_program_u8x4_kernel
// reads them (N = 4: twelve bytes = three dwords per thread and trip, the last count % 4 pixels byte by byte) or, for a uniform batch
// whose images do not start on dwords, one pixel per thread (N = 1).  A workgroup counts into its own 256 bins in LDS (ds_add_u32) and
// adds the occupied ones to the image's row with one global atomicAdd each: sums of integers, the same in any order.
template <class Imgs, int N>
__global__ __launch_bounds__(256) void program_hist_u8_kernel(const unsigned char* __restrict__ x, Imgs imgs, const int* __restrict__ ops,
                                                              const double* __restrict__ args, const unsigned char* __restrict__ luts,
                                                              const int* __restrict__ stop, const int* __restrict__ channel,
                                                              unsigned int* __restrict__ hist) {
    const int img = blockIdx.y;
    int n_steps = stop[img];
    if (n_steps < 0) return;                                            // the same for the whole workgroup, in front of every barrier
    n_steps = n_steps < IMG_PROG ? n_steps : IMG_PROG;
    __shared__ int sdiv[256], hdiv[256];
    __shared__ unsigned int slut[IMG_LUT_SLOTS * 64];
    __shared__ unsigned int h[256];
    sdiv[threadIdx.x] = img_div_table(255 << 12, (int)threadIdx.x, 1);
    hdiv[threadIdx.x] = img_div_table(180 << 12, (int)threadIdx.x, 6);
    if (luts) slut[threadIdx.x] = reinterpret_cast<const unsigned int*>(luts)[(size_t)img * IMG_LUT_SLOTS * 64 + threadIdx.x];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned char* lut = luts ? reinterpret_cast<const unsigned char*>(slut) : nullptr;
    const int* op = ops + (size_t)img * IMG_PROG;
    const double* arg = args + (size_t)img * IMG_PROG;
    const int ch = channel[img];
    const long long pixels = imgs.count(img), off = imgs.offset(img);
    const long long groups = pixels / N, items = groups + (pixels - groups * N);
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < items; g += (long long)gridDim.x * 256) {
        if (N == 1 || g >= groups) {                                     // one pixel
            const size_t e = (size_t)(N == 1 ? g : groups * N + (g - groups)) * 3;
            double px[1][3] = {{(double)x[off + e], (double)x[off + e + 1], (double)x[off + e + 2]}};
            int tag = IMG_U8;
            for (int k = 0; k < n_steps; ++k) {
                const int o = op[k];
                if (o == OP_END) break;
                img_apply<1>(px, tag, o, arg[k], sdiv, hdiv, lut);
            }
            atomicAdd(&h[(int)(ch == 0 ? px[0][0] : (ch == 1 ? px[0][1] : px[0][2])) & 255], 1u);
            continue;
        }
        const unsigned int* xw = reinterpret_cast<const unsigned int*>(x + off);
        const size_t e = (size_t)g * 3;
        const unsigned int w0 = xw[e], w1 = xw[e + 1], w2 = xw[e + 2];
        double px[4][3];
        px[0][0] = w0 & 255u; px[0][1] = (w0 >> 8) & 255u; px[0][2] = (w0 >> 16) & 255u;
        px[1][0] = w0 >> 24; px[1][1] = w1 & 255u; px[1][2] = (w1 >> 8) & 255u;
        px[2][0] = (w1 >> 16) & 255u; px[2][1] = w1 >> 24; px[2][2] = w2 & 255u;
        px[3][0] = (w2 >> 8) & 255u; px[3][1] = (w2 >> 16) & 255u; px[3][2] = w2 >> 24;
        int tag = IMG_U8;
        for (int k = 0; k < n_steps; ++k) {
            const int o = op[k];
            if (o == OP_END) break;
            img_apply<4>(px, tag, o, arg[k], sdiv, hdiv, lut);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) atomicAdd(&h[(int)(ch == 0 ? px[n][0] : (ch == 1 ? px[n][1] : px[n][2])) & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[(size_t)img * 256 + threadIdx.x], h[threadIdx.x]);
}

// cv2.equalizeHist's second half for a batch: hist [B][256] -> luts[i][slot[i]][256] (slot[i] < 0: image i is skipped), the rule of
// data_generator/_image_ops.equalize_table: bins up to the first occupied one -> 0, the others -> the count of the pixels in the bins
// behind the first occupied one up to theirs, times the float32 scale 255.f / (total - hist[first]), float32 product, rounded to nearest
// even, clamped; one occupied bin (or none): the identity.  ONE WAVE per image: lane l holds bins 4 l .. 4 l + 3, a shuffle scan over
// the lanes' sums gives every bin its cumulative count, and each lane stores its four table bytes as one dword.
__global__ __launch_bounds__(64) void equalize_tables_kernel(const unsigned int* __restrict__ hist, const int* __restrict__ slot,
                                                             unsigned char* __restrict__ luts) {
    const int img = blockIdx.x, lane = threadIdx.x;
    const int s = slot[img];
    if (s < 0 || s >= IMG_LUT_SLOTS) return;
    const uint4 hv = reinterpret_cast<const uint4*>(hist + (size_t)img * 256)[lane];
    const u64 hb[4] = {hv.x, hv.y, hv.z, hv.w};
    const u64 mine = hb[0] + hb[1] + hb[2] + hb[3];
    u64 incl = mine;                                                    // inclusive scan of the lanes' sums
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const u64 total = __shfl(incl, 63);
    int first = hv.x ? 4 * lane : (hv.y ? 4 * lane + 1 : (hv.z ? 4 * lane + 2 : (hv.w ? 4 * lane + 3 : 256)));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) first = min(first, __shfl_xor(first, d));
    const int fq = first & 3;
    const u64 h_first = __shfl(fq == 0 ? hb[0] : (fq == 1 ? hb[1] : (fq == 2 ? hb[2] : hb[3])), (first >> 2) & 63);
    unsigned int packed = 0u;
    if (first == 256 || h_first == total) {                             // a constant plane is left alone
#pragma unroll
        for (int j = 0; j < 4; ++j) packed |= (unsigned int)(4 * lane + j) << (8 * j);
    } else {
        const float scale = 255.f / (float)(total - h_first);
        u64 cum = incl - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cum += hb[j];
            const u64 below = (4 * lane + j <= first) ? 0ull : cum - h_first;
            const float r = rintf((float)below * scale);
            packed |= (unsigned int)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r)) << (8 * j);
        }
    }
    reinterpret_cast<unsigned int*>(luts + ((size_t)img * IMG_LUT_SLOTS + s) * 256)[lane] = packed;
}

}  // namespace ssdhip

using namespace ssdhip;

static unsigned img_blocks(long long work, unsigned cap) {
    long long b = (work + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// The check of a batch's programs while they are still on the HOST (the launching exports get them on the device and only enqueue):
// every op code known; OP_LUT only with tables (have_luts), on a uint8 state, with slot + 4 * mask, mask 1 .. 7.
extern "C" int ssdhip_image_program_check(const int* ops_host, const double* args_host, int n_images, int in_dtype, int have_luts) {
    if (!ops_host || !args_host || n_images <= 0 || in_dtype < IMG_U8 || in_dtype > IMG_F64) return SSDHIP_E_BADARG;
    for (int i = 0; i < n_images; ++i) {
        int tag = in_dtype;
        for (int k = 0; k < IMG_PROG; ++k) {
            const int o = ops_host[(size_t)i * IMG_PROG + k];
            if (o == OP_END) break;
            if (o < OP_END || o > OP_LUT) return SSDHIP_E_BADARG;
            if (o == OP_LUT) {
                const double a = args_host[(size_t)i * IMG_PROG + k];
                if (!have_luts || tag != IMG_U8 || !(a >= 4.0 && a <= 31.0) || a != (double)(int)a) return SSDHIP_E_BADARG;
            }
            if (o == OP_TO_F32) tag = IMG_F32;
            else if (o == OP_TO_U8) tag = IMG_U8;
            else if ((o == OP_BRIGHTNESS || o == OP_CONTRAST) && tag != IMG_F32) tag = IMG_F64;
        }
    }
    return SSDHIP_OK;
}

extern "C" int ssdhip_image_program_lut(const void* x, int in_dtype, void* y, int out_dtype, int n_images, long long pixels_per_image,
                                        const int* ops_dev, const double* args_dev, const void* luts_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !y || !ops_dev || !args_dev || n_images <= 0 || n_images > 65535 || pixels_per_image <= 0) return SSDHIP_E_BADARG;
    if (in_dtype < IMG_U8 || in_dtype > IMG_F64 || out_dtype < IMG_U8 || out_dtype > IMG_F64 || ((uintptr_t)luts_dev & 3)) return SSDHIP_E_BADARG;
    const unsigned char* luts = static_cast<const unsigned char*>(luts_dev);
    if (in_dtype == IMG_U8 && out_dtype == IMG_U8 && pixels_per_image % 4 == 0 && !(((uintptr_t)x | (uintptr_t)y) & 3)) {
        hipLaunchKernelGGL(pixel_program_u8x4_kernel<UniformImages>, dim3(img_blocks(pixels_per_image / 4, 2048), n_images), dim3(256), 0,
                           stream, static_cast<const unsigned char*>(x), static_cast<unsigned char*>(y), UniformImages{pixels_per_image},
                           ops_dev, args_dev, luts);
        return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
    }
    hipLaunchKernelGGL(pixel_program_kernel, dim3(img_blocks(pixels_per_image, 4096), n_images), dim3(256), 0, stream, x, in_dtype, y, out_dtype,
                       pixels_per_image, ops_dev, args_dev, luts);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_image_program(const void* x, int in_dtype, void* y, int out_dtype, int n_images, long long pixels_per_image,
                                    const int* ops_dev, const double* args_dev, void* stream_) {
    return ssdhip_image_program_lut(x, in_dtype, y, out_dtype, n_images, pixels_per_image, ops_dev, args_dev, nullptr, stream_);
}

extern "C" int ssdhip_image_resize_cv_u8(const void* x, void* y, int B, int H, int W, int Ho, int Wo, int C, int kind, int area,
                                         const int* ix_dev, const double* wx_dev, int nx, const int* iy_dev, const double* wy_dev, int ny,
                                         void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !y || !ix_dev || !wx_dev || !iy_dev || !wy_dev) return SSDHIP_E_BADARG;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || Ho <= 0 || Ho > 65535 || Wo <= 0 || C <= 0 || C > 4 || nx <= 0 || ny <= 0 || nx > 64 ||
        ny > 64 || kind < 0 || kind > CV_COPY || area < 1)
        return SSDHIP_E_BADARG;
    if ((kind == CV_LINEAR && (nx != 2 || ny != 2)) || ((kind == CV_NEAREST || kind == CV_COPY) && (nx != 1 || ny != 1))) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(resize_cv_kernel, dim3((unsigned)((Wo * C + 255) / 256), (unsigned)Ho, (unsigned)B), dim3(256), 0, stream,
                       static_cast<const unsigned char*>(x), static_cast<unsigned char*>(y), H, W, Ho, Wo, C, kind, area, ix_dev, wx_dev, nx,
                       iy_dev, wy_dev, ny);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_image_resize_gather_cv_u8(const void* x, void* y, int B, int H, int W, int Ho, int Wo, int C, const int* plan_dev,
                                                const int* ix_dev, const double* wx_dev, int nx, const int* iy_dev, const double* wy_dev,
                                                int ny, const void* background_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !y || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || !background_dev) return SSDHIP_E_BADARG;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || Ho <= 0 || Ho > 65535 || Wo <= 0 || C <= 0 || C > 4 || nx < 2 || ny < 2 || nx > 64 || ny > 64)
        return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(resize_gather_cv_kernel<UniformGatherSrc>, dim3((unsigned)((Wo * C + 255) / 256), (unsigned)Ho, (unsigned)B), dim3(256),
                       0, stream, UniformGatherSrc{static_cast<const unsigned char*>(x), H, W, C}, static_cast<unsigned char*>(y), Ho, Wo, C,
                       plan_dev, ix_dev, wx_dev, nx, iy_dev, wy_dev, ny, static_cast<const unsigned char*>(background_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// ---- ragged batches: B uint8 images of different sizes in one buffer, table [B][4] int64 = byte offset, H, W, C ----------------------
// The gather of ssdhip_image_resize_gather_cv_u8 with each image read through its table entry and ConvertTo3Channels folded into the read
// (C = 1 replicated, C = 4 alpha dropped): y [B][Ho][Wo][3].  The tables' indices address each image's own rows / columns.
extern "C" int ssdhip_image_resize_gather_ragged_u8(const void* x, const long long* table_dev, void* y, int B, int Ho, int Wo,
                                                    const int* plan_dev, const int* ix_dev, const double* wx_dev, int nx, const int* iy_dev,
                                                    const double* wy_dev, int ny, const void* background_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !table_dev || !y || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || !background_dev) return SSDHIP_E_BADARG;
    if (B <= 0 || B > 65535 || Ho <= 0 || Ho > 65535 || Wo <= 0 || Wo > (1 << 24) || nx < 2 || ny < 2 || nx > 64 || ny > 64)
        return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(resize_gather_cv_kernel<RaggedGatherSrc>, dim3((unsigned)((Wo * 3 + 255) / 256), (unsigned)Ho, (unsigned)B), dim3(256),
                       0, stream, RaggedGatherSrc{static_cast<const unsigned char*>(x), table_dev}, static_cast<unsigned char*>(y), Ho, Wo,
                       3, plan_dev, ix_dev, wx_dev, nx, iy_dev, wy_dev, ny, static_cast<const unsigned char*>(background_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// The two gathers above for plans with quarter turns (ssdhip_sat_augment_plans[_ragged]): transposed_dev [B] swaps image b's source
// address, index -2 reads 0.
extern "C" int ssdhip_image_resize_gather_turn_cv_u8(const void* x, void* y, int B, int H, int W, int Ho, int Wo, int C, const int* plan_dev,
                                                     const int* ix_dev, const double* wx_dev, int nx, const int* iy_dev,
                                                     const double* wy_dev, int ny, const int* transposed_dev, const void* background_dev,
                                                     void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !y || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || !transposed_dev || !background_dev) return SSDHIP_E_BADARG;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || Ho <= 0 || Ho > 65535 || Wo <= 0 || C <= 0 || C > 4 || nx < 2 || ny < 2 || nx > 64 || ny > 64)
        return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(resize_gather_turn_cv_kernel<UniformGatherSrc>, dim3((unsigned)((Wo * C + 255) / 256), (unsigned)Ho, (unsigned)B),
                       dim3(256), 0, stream, UniformGatherSrc{static_cast<const unsigned char*>(x), H, W, C}, static_cast<unsigned char*>(y),
                       Ho, Wo, C, plan_dev, ix_dev, wx_dev, nx, iy_dev, wy_dev, ny, transposed_dev,
                       static_cast<const unsigned char*>(background_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_image_resize_gather_turn_ragged_u8(const void* x, const long long* table_dev, void* y, int B, int Ho, int Wo,
                                                         const int* plan_dev, const int* ix_dev, const double* wx_dev, int nx,
                                                         const int* iy_dev, const double* wy_dev, int ny, const int* transposed_dev,
                                                         const void* background_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !table_dev || !y || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || !transposed_dev || !background_dev)
        return SSDHIP_E_BADARG;
    if (B <= 0 || B > 65535 || Ho <= 0 || Ho > 65535 || Wo <= 0 || Wo > (1 << 24) || nx < 2 || ny < 2 || nx > 64 || ny > 64)
        return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(resize_gather_turn_cv_kernel<RaggedGatherSrc>, dim3((unsigned)((Wo * 3 + 255) / 256), (unsigned)Ho, (unsigned)B),
                       dim3(256), 0, stream, RaggedGatherSrc{static_cast<const unsigned char*>(x), table_dev}, static_cast<unsigned char*>(y),
                       Ho, Wo, 3, plan_dev, ix_dev, wx_dev, nx, iy_dev, wy_dev, ny, transposed_dev,
                       static_cast<const unsigned char*>(background_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// The photometric programs of ssdhip_image_program (uint8 -> uint8) on a ragged batch of 3-channel images, one program per image, ONE
// launch: y has x's layout (the same table); max_pixels = the largest H W of the batch (sizes the grid).
extern "C" int ssdhip_image_program_ragged_lut_u8(const void* x, const long long* table_dev, void* y, int B, long long max_pixels,
                                                  const int* ops_dev, const double* args_dev, const void* luts_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !table_dev || !y || !ops_dev || !args_dev || B <= 0 || B > 65535 || max_pixels <= 0) return SSDHIP_E_BADARG;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)luts_dev) & 3) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(pixel_program_u8x4_kernel<RaggedImages>, dim3(img_blocks((max_pixels + 3) / 4, 2048), B), dim3(256), 0, stream,
                       static_cast<const unsigned char*>(x), static_cast<unsigned char*>(y), RaggedImages{table_dev}, ops_dev, args_dev,
                       static_cast<const unsigned char*>(luts_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_image_program_ragged_u8(const void* x, const long long* table_dev, void* y, int B, long long max_pixels,
                                              const int* ops_dev, const double* args_dev, void* stream_) {
    return ssdhip_image_program_ragged_lut_u8(x, table_dev, y, B, max_pixels, ops_dev, args_dev, nullptr, stream_);
}

// The histograms of one channel of a batch in the middle of its programs (program_hist_u8_kernel): table_dev = the ragged batch's table
// and `pixels` its largest H W, or table_dev NULL: B images of `pixels` pixels each, (B, H, W, 3).  hist_dev [B][256] is zeroed here.
extern "C" int ssdhip_image_program_hist_u8(const void* x, const long long* table_dev, int B, long long pixels, const int* ops_dev,
                                            const double* args_dev, const void* luts_dev, const int* stop_dev, const int* channel_dev,
                                            unsigned int* hist_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !ops_dev || !args_dev || !stop_dev || !channel_dev || !hist_dev || B <= 0 || B > 65535 || pixels <= 0) return SSDHIP_E_BADARG;
    if ((uintptr_t)luts_dev & 3) return SSDHIP_E_BADARG;
    if (table_dev && ((uintptr_t)x & 3)) return SSDHIP_E_BADARG;
    if (zero_async(hist_dev, (size_t)B * 256 * sizeof(unsigned int), stream) != hipSuccess) return SSDHIP_E_LAUNCH;
    const unsigned char* xs = static_cast<const unsigned char*>(x);
    const unsigned char* luts = static_cast<const unsigned char*>(luts_dev);
    if (table_dev)
        hipLaunchKernelGGL((program_hist_u8_kernel<RaggedImages, 4>), dim3(img_blocks((pixels + 3) / 4, 64), B), dim3(256), 0, stream, xs,
                           RaggedImages{table_dev}, ops_dev, args_dev, luts, stop_dev, channel_dev, hist_dev);
    else if (pixels % 4 == 0 && !((uintptr_t)x & 3))
        hipLaunchKernelGGL((program_hist_u8_kernel<UniformImages, 4>), dim3(img_blocks(pixels / 4, 64), B), dim3(256), 0, stream, xs,
                           UniformImages{pixels}, ops_dev, args_dev, luts, stop_dev, channel_dev, hist_dev);
    else
        hipLaunchKernelGGL((program_hist_u8_kernel<UniformImages, 1>), dim3(img_blocks(pixels, 64), B), dim3(256), 0, stream, xs,
                           UniformImages{pixels}, ops_dev, args_dev, luts, stop_dev, channel_dev, hist_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_image_equalize_tables(const unsigned int* hist_dev, const int* slot_dev, void* luts_dev, int B, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!hist_dev || !slot_dev || !luts_dev || B <= 0 || ((uintptr_t)hist_dev & 15) || ((uintptr_t)luts_dev & 3)) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(equalize_tables_kernel, dim3((unsigned)B), dim3(64), 0, stream, hist_dev, slot_dev, static_cast<unsigned char*>(luts_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_image_hist_u8(const void* x, long long n_pixels, int C, int channel, unsigned int* hist_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !hist_dev || n_pixels <= 0 || C <= 0 || channel < 0 || channel >= C) return SSDHIP_E_BADARG;
    if (zero_async(hist_dev, 256 * sizeof(unsigned int), stream) != hipSuccess) return SSDHIP_E_LAUNCH;
    hipLaunchKernelGGL(hist_u8_kernel, dim3(img_blocks(n_pixels, 1024)), dim3(256), 0, stream, static_cast<const unsigned char*>(x), n_pixels, C,
                       channel, hist_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_image_lut_u8(const void* x, void* y, long long n_values, int C, int channel_mask, const void* table_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!x || !y || !table_dev || n_values <= 0 || C <= 0 || C > 8) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(lut_u8_kernel, dim3(img_blocks(n_values, 4096)), dim3(256), 0, stream, static_cast<const unsigned char*>(x),
                       static_cast<unsigned char*>(y), n_values, C, channel_mask, static_cast<const unsigned char*>(table_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
