// Baseline JPEG decoding of a batch on the device, bit for bit what libjpeg(-turbo) returns with its default settings (the "islow"
// IDCT, "fancy" chroma upsampling, the 16-bit fixed-point YCbCr -> RGB tables): data_generator/jpeg_decode.py parses the markers on
// the host and uploads ONE descriptor buffer; three launches turn it into the images.
//   1. jpeg_entropy_kernel  one LANE per (image, restart segment): csrc/ssdhip_jpeg_entropy.h, int16 coefficients [block][64]
//                           (with an entry-point index: jpeg_entropy_entry_kernel + jpeg_entropy_record_kernel, section 1' below);
//   2. jpeg_block_kernel    one thread per 8 x 8 block, the block in registers: dequantise, IDCT, range limit -> sample planes,
//                           one per component, padded to whole blocks;
//   3. jpeg_pixel_kernel    one thread per output pixel: upsample the chroma planes, convert, crop to H x W, store into the image's
//                           slot of the output buffer (grayscale: the luma plane).
// Nothing is cleared in front of a launch: the entropy lanes zero-fill the blocks they decode, every sample and pixel is written,
// and the status words come up as zeros WITH the descriptors and only ever receive non-zero ordinary stores.  An image whose status
// ends non-zero is decoded by the host decoder instead (its pixels here are then whatever the stages made of the partial data).
#include <hip/hip_runtime.h>

#include "ssdhip.h"
#include "ssdhip_jpeg_entropy.h"

namespace {

static_assert(sizeof(ssdhip_jpeg_image) == 4 * SSDHIP_JPEG_IMAGE_WORDS, "image descriptor layout");
static_assert(sizeof(ssdhip_jpeg_segment) == 4 * SSDHIP_JPEG_SEGMENT_WORDS, "segment descriptor layout");
static_assert(sizeof(ssdhip_jpeg_huff) == SSDHIP_JPEG_HUFF_BYTES, "Huffman table layout");
static_assert(sizeof(ssdhip_jpeg_entry) == 4 * SSDHIP_JPEG_ENTRY_WORDS, "entry layout");

struct JpegBatch {
    const ssdhip_jpeg_image* images;
    const ssdhip_jpeg_segment* segments;
    const unsigned short* qt;          // [n_qt][64], natural order
    const ssdhip_jpeg_huff* huff;
    const unsigned char* data;
    int* status;                       // [n_images]
    int n_images, n_segments, n_qt, n_huff, data_bytes;
    long long total_blocks, out_bytes;
};

__device__ __forceinline__ bool jpeg_geometry_ok(const ssdhip_jpeg_image& im) {
    return (im.ncomp == 1 || im.ncomp == 3) && im.hs >= 1 && im.hs <= 2 && im.vs >= 1 && im.vs <= im.hs &&
           (im.ncomp == 3 || (im.hs == 1 && im.vs == 1)) && im.mcux >= 1 && im.mcuy >= 1 && im.mcux <= 8192 && im.mcuy <= 8192 &&
           im.height >= 1 && im.width >= 1 && im.height <= im.mcuy * im.vs * 8 && im.width <= im.mcux * im.hs * 8 && im.coef_base >= 0;
}

__device__ __forceinline__ int jpeg_blocks(const ssdhip_jpeg_image& im) {
    return im.mcux * im.mcuy * (im.hs * im.vs + (im.ncomp == 3 ? 2 : 0));
}

// ---- 1. entropy: `lanes` segments per 64-lane workgroup (the host spreads few segments over many waves: a lane that shares its wave
// with lanes at other points of the decoder pays for their branches) -----------------------------------------------------------------
__global__ void __launch_bounds__(64) jpeg_entropy_kernel(JpegBatch b, int lanes, short* coef) {
    const int lane = threadIdx.x;
    if (lane >= lanes) return;
    const long long s = (long long)blockIdx.x * lanes + lane;
    if (s >= b.n_segments) return;
    const ssdhip_jpeg_segment seg = b.segments[s];
    if (seg.image < 0 || seg.image >= b.n_images) return;        // no image to blame: the host checks the table it builds
    const int st = ssdhip_jpeg_decode_segment(b.images + seg.image, &seg, b.huff, b.n_huff, b.data, b.data_bytes, coef, b.total_blocks);
    if (st != 0) b.status[seg.image] = st;
}

// ---- 1'. entropy with an entry-point index (ssdhip_jpeg_decode_batch_indexed) -----------------------------------------------------------
// A file without restart markers is one segment, hence one lane of the kernel above.  Its MCU rows can be decoded by a lane each once
// the host knows where every row starts: the RECORD kernel decodes such a file sequentially, once, and writes those entries; from
// then on the ENTRY kernel decodes it with one lane per entry, every lane checking that it ends on the next entry (header comment of
// ssdhip_jpeg_entropy.h: a wrong entry can only set the status, never yield other coefficients).
// modes[image]: low 2 bits 0 = the per-segment path, 1 = indexed, 2 = record; the bits above: for 1 the image's segment, for 2 the
// image's first row in the checkpoint buffer.
struct JpegIndexArgs {
    const ssdhip_jpeg_entry* entries;  // [n_entries], an image's entries in a row, in MCU order
    const int* modes;                  // [n_images]
    ssdhip_jpeg_entry* ckpt;           // [ckpt_entries]
    int n_entries, ckpt_entries;
};

__global__ void __launch_bounds__(64) jpeg_entropy_entry_kernel(JpegBatch b, JpegIndexArgs x, int lanes, short* coef) {
    const int lane = threadIdx.x;
    if (lane >= lanes) return;
    const long long e = (long long)blockIdx.x * lanes + lane;
    if (e >= x.n_entries) return;
    const ssdhip_jpeg_entry entry = x.entries[e];
    if (entry.image < 0 || entry.image >= b.n_images) return;    // no image to blame: the host checks the table it builds
    const int mode = x.modes[entry.image];
    const int s = mode >> 2;
    int st;
    if ((mode & 3) != 1 || s < 0 || s >= b.n_segments || b.segments[s].image != entry.image) {
        st = SSDHIP_JPEG_ST_DESC;
    } else {
        const ssdhip_jpeg_segment seg = b.segments[s];
        const bool first = e == 0 || x.entries[e - 1].image != entry.image;
        const bool last = e + 1 >= x.n_entries || x.entries[e + 1].image != entry.image;
        ssdhip_jpeg_entry next = entry;
        if (!last) next = x.entries[e + 1];
        st = ssdhip_jpeg_decode_span(b.images + entry.image, &seg, &entry, last ? nullptr : &next, first ? 1 : 0, b.huff, b.n_huff, b.data,
                                     b.data_bytes, coef, b.total_blocks, nullptr, 0);
    }
    if (st != 0) b.status[entry.image] = st;
}

// One lane per segment of the images the entry kernel does not decode: the per-segment path as it is, or (mode 2) the same sequential
// decode that also records the image's entries, one per MCU row, at ckpt[the image's first row + MCU row].
__global__ void __launch_bounds__(64) jpeg_entropy_record_kernel(JpegBatch b, JpegIndexArgs x, int lanes, short* coef) {
    const int lane = threadIdx.x;
    if (lane >= lanes) return;
    const long long s = (long long)blockIdx.x * lanes + lane;
    if (s >= b.n_segments) return;
    const ssdhip_jpeg_segment seg = b.segments[s];
    if (seg.image < 0 || seg.image >= b.n_images) return;
    const int mode = x.modes[seg.image];
    if ((mode & 3) == 1) return;                                 // the entry kernel's
    int st;
    if ((mode & 3) == 2) {
        const int base = mode >> 2;
        if (base < 0 || base >= x.ckpt_entries)
            st = SSDHIP_JPEG_ST_DESC;
        else
            st = ssdhip_jpeg_decode_span(b.images + seg.image, &seg, nullptr, nullptr, 0, b.huff, b.n_huff, b.data, b.data_bytes, coef,
                                         b.total_blocks, x.ckpt + base, x.ckpt_entries - base);
    } else {
        st = ssdhip_jpeg_decode_segment(b.images + seg.image, &seg, b.huff, b.n_huff, b.data, b.data_bytes, coef, b.total_blocks);
    }
    if (st != 0) b.status[seg.image] = st;
}

// ---- 2. blocks: jidctint's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2) ---------------------------------------------------------------
#define JPEG_GUARD 12287   // |dequantised| and |pass-1 value| of an 8-bit image stay far below; inside it every sum below fits 32 bits

__device__ __forceinline__ void jpeg_idct_1d(const int (&in)[8], int (&out)[8], int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137);
    int tmp3 = z1 + z2 * 6270;
    z2 = in[0], z3 = in[4];
    int tmp0 = (z2 + z3) * 8192;
    int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const int round = 1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + round) >> shift;
    out[7] = (tmp10 - tmp3 + round) >> shift;
    out[1] = (tmp11 + tmp2 + round) >> shift;
    out[6] = (tmp11 - tmp2 + round) >> shift;
    out[2] = (tmp12 + tmp1 + round) >> shift;
    out[5] = (tmp12 - tmp1 + round) >> shift;
    out[3] = (tmp13 + tmp0 + round) >> shift;
    out[4] = (tmp13 - tmp0 + round) >> shift;
}

__device__ __forceinline__ unsigned int jpeg_range_limit(int v) {
    const int i = (v + 128) & 1023;                              // libjpeg's post-IDCT table: 0..255, 255 up to 639, 0 behind
    return i < 256 ? (unsigned int)i : (i < 640 ? 255u : 0u);
}

__global__ void __launch_bounds__(256) jpeg_block_kernel(JpegBatch b, const short* coef, unsigned char* planes) {
    const int image = blockIdx.y;
    const ssdhip_jpeg_image im = b.images[image];
    if (!jpeg_geometry_ok(im) || (long long)im.coef_base + jpeg_blocks(im) > b.total_blocks) {
        if (blockIdx.x == 0 && threadIdx.x == 0) b.status[image] = SSDHIP_JPEG_ST_DESC;
        return;
    }
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= jpeg_blocks(im)) return;
    const int n0 = im.mcux * im.hs * im.mcuy * im.vs, n1 = im.mcux * im.mcuy;
    const int c = blk < n0 ? 0 : (blk < n0 + n1 ? 1 : 2);
    const int in_grid = blk - (c == 0 ? 0 : (c == 1 ? n0 : n0 + n1));
    const int grid_w = c == 0 ? im.mcux * im.hs : im.mcux;
    const int by = in_grid / grid_w, bx = in_grid - by * grid_w;
    int q = c == 0 ? im.qt[0] : (c == 1 ? im.qt[1] : im.qt[2]);
    q = q < 0 ? 0 : (q >= b.n_qt ? b.n_qt - 1 : q);

    const long long block = (long long)im.coef_base + blk;
    const uint4* src = reinterpret_cast<const uint4*>(coef + block * 64);
    const uint4* qsrc = reinterpret_cast<const uint4*>(b.qt + q * 64);
    int v[64];
    bool wild = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 cw = src[r], qw = qsrc[r];
        const unsigned int cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d0 = (int)(short)(cs[k] & 0xFFFFu) * (int)(qs[k] & 0xFFFFu);
            const int d1 = (int)(short)(cs[k] >> 16) * (int)(qs[k] >> 16);
            wild = wild || d0 > JPEG_GUARD || d0 < -JPEG_GUARD || d1 > JPEG_GUARD || d1 < -JPEG_GUARD;
            v[r * 8 + 2 * k] = min(max(d0, -JPEG_GUARD), JPEG_GUARD);
            v[r * 8 + 2 * k + 1] = min(max(d1, -JPEG_GUARD), JPEG_GUARD);
        }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {                          // pass 1: columns
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = v[r * 8 + col];
        jpeg_idct_1d(in, out, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            wild = wild || out[r] > JPEG_GUARD || out[r] < -JPEG_GUARD;
            v[r * 8 + col] = min(max(out[r], -JPEG_GUARD), JPEG_GUARD);
        }
    }
    unsigned char* plane = planes + ((long long)im.coef_base + (c == 0 ? 0 : (c == 1 ? n0 : n0 + n1))) * 64;
    const long long stride = (long long)grid_w * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                                // pass 2: rows, range limit, 8 samples = one 8-byte store
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = v[r * 8 + k];
        jpeg_idct_1d(in, out, 18);
        uint2 px;
        px.x = jpeg_range_limit(out[0]) | (jpeg_range_limit(out[1]) << 8) | (jpeg_range_limit(out[2]) << 16) | (jpeg_range_limit(out[3]) << 24);
        px.y = jpeg_range_limit(out[4]) | (jpeg_range_limit(out[5]) << 8) | (jpeg_range_limit(out[6]) << 16) | (jpeg_range_limit(out[7]) << 24);
        *reinterpret_cast<uint2*>(plane + ((long long)by * 8 + r) * stride + (long long)bx * 8) = px;
    }
    if (wild) b.status[image] = SSDHIP_JPEG_ST_RANGE;
}

// ---- 3. pixels: jdsample's fancy upsampling + jdcolor's YCbCr -> RGB ---------------------------------------------------------------------
// One chroma sample at output pixel (y, x).  (cw, ch): the component's downsampled size ceil(W / hs), ceil(H / vs), at which the edges
// replicate; libjpeg takes the fancy (triangle) filter only for cw > 2 and replicates the sample otherwise.
__device__ __forceinline__ int jpeg_chroma(const unsigned char* p, long long stride, int y, int x, int hs, int vs, int cw, int ch) {
    if (hs == 1) return p[(long long)y * stride + x];            // (vs == 1: the plan admits 1x1, 2x1, 2x2)
    const int c = x >> 1;
    if (cw <= 2) return p[(long long)(vs == 2 ? y >> 1 : y) * stride + c];
    const int left = c > 0 ? c - 1 : 0, right = c < cw - 1 ? c + 1 : cw - 1;
    if (vs == 1) {                                               // h2v1: (3 c + l + 1) >> 2, (3 c + r + 2) >> 2, ends copied
        const unsigned char* row = p + (long long)y * stride;
        const int cur = row[c];
        if (x & 1) return c == cw - 1 ? cur : (3 * cur + row[right] + 2) >> 2;
        return c == 0 ? cur : (3 * cur + row[left] + 1) >> 2;
    }
    const int cy = y >> 1;                                       // h2v2: 3 near + far per column, then the same filter at 1/16
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const unsigned char* near = p + (long long)cy * stride;
    const unsigned char* far = p + (long long)fy * stride;
    const int cur = 3 * near[c] + far[c];
    if (x & 1) return c == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * near[right] + far[right] + 7) >> 4;
    return c == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * near[left] + far[left] + 8) >> 4;
}

__device__ __forceinline__ unsigned char jpeg_clamp(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ void __launch_bounds__(256) jpeg_pixel_kernel(JpegBatch b, const unsigned char* planes, unsigned char* out) {
    const int image = blockIdx.y;
    const ssdhip_jpeg_image im = b.images[image];
    const long long n_px = (long long)im.height * im.width;
    if (!jpeg_geometry_ok(im) || (long long)im.coef_base + jpeg_blocks(im) > b.total_blocks || im.out_offset < 0 ||
        im.out_offset + n_px * im.ncomp > b.out_bytes) {
        if (blockIdx.x == 0 && threadIdx.x == 0) b.status[image] = SSDHIP_JPEG_ST_DESC;
        return;
    }
    const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
    if (px >= n_px) return;
    const int y = (int)(px / im.width), x = (int)(px - (long long)y * im.width);
    const int n0 = im.mcux * im.hs * im.mcuy * im.vs, n1 = im.mcux * im.mcuy;
    const unsigned char* p0 = planes + (long long)im.coef_base * 64;
    const long long s0 = (long long)im.mcux * im.hs * 8;
    const int lum = p0[(long long)y * s0 + x];
    unsigned char* dst = out + im.out_offset + px * im.ncomp;
    if (im.ncomp == 1) {
        dst[0] = (unsigned char)lum;
        return;
    }
    const long long s1 = (long long)im.mcux * 8;
    const int cw = (im.width + im.hs - 1) / im.hs, ch = (im.height + im.vs - 1) / im.vs;
    const int cb = jpeg_chroma(p0 + (long long)n0 * 64, s1, y, x, im.hs, im.vs, cw, ch) - 128;
    const int cr = jpeg_chroma(p0 + ((long long)n0 + n1) * 64, s1, y, x, im.hs, im.vs, cw, ch) - 128;
    dst[0] = jpeg_clamp(lum + ((91881 * cr + 32768) >> 16));
    dst[1] = jpeg_clamp(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    dst[2] = jpeg_clamp(lum + ((116130 * cb + 32768) >> 16));
}

}  // namespace

extern "C" int ssdhip_jpeg_layout(int* words) {
    if (!words) return SSDHIP_E_BADARG;
    words[0] = SSDHIP_JPEG_IMAGE_WORDS, words[1] = SSDHIP_JPEG_SEGMENT_WORDS, words[2] = SSDHIP_JPEG_HUFF_BYTES, words[3] = 256;
    return SSDHIP_OK;
}

extern "C" int ssdhip_jpeg_entry_layout(int* words) {
    if (!words) return SSDHIP_E_BADARG;
    words[0] = SSDHIP_JPEG_ENTRY_WORDS, words[1] = SSDHIP_JPEG_ST_INDEX;
    return SSDHIP_OK;
}

namespace {

// Both exports: check the arguments, then stage 1 (the per-segment kernel, or with `x` the entry and record kernels), 2 and 4.
int jpeg_decode_batch(void* desc_dev, long long desc_bytes, int n_images, int n_segments, int n_qt, int n_huff, int off_images,
                      int off_segments, int off_qt, int off_huff, int off_data, int data_bytes, int off_status, int max_blocks,
                      int max_pixels, long long total_blocks, int lanes_per_wave, int stages, void* coef_dev, void* planes_dev,
                      void* out_dev, long long out_bytes, hipStream_t stream, bool indexed, int off_entries, int n_entries, int off_modes,
                      void* ckpt_dev, int ckpt_entries, int record_segments, int entry_lanes_per_wave) {
    if (!desc_dev || !coef_dev || !planes_dev || !out_dev || n_images <= 0 || n_images > 65535 || n_segments <= 0 || n_qt <= 0 ||
        n_huff <= 0 || data_bytes < 0 || max_blocks <= 0 || max_pixels <= 0 || total_blocks <= 0 || out_bytes <= 0 ||
        lanes_per_wave < 1 || lanes_per_wave > 64 || (stages & ~7) != 0)
        return SSDHIP_E_BADARG;
    const long long parts[8][2] = {{off_images, 4LL * SSDHIP_JPEG_IMAGE_WORDS * n_images},
                                   {off_segments, 4LL * SSDHIP_JPEG_SEGMENT_WORDS * n_segments},
                                   {off_qt, 128LL * n_qt},
                                   {off_huff, (long long)SSDHIP_JPEG_HUFF_BYTES * n_huff},
                                   {off_data, data_bytes},
                                   {off_status, 4LL * n_images},
                                   {off_entries, 4LL * SSDHIP_JPEG_ENTRY_WORDS * n_entries},
                                   {off_modes, 4LL * n_images}};
    for (int k = 0; k < (indexed ? 8 : 6); ++k)
        if (parts[k][0] < 0 || (parts[k][0] & 15) != 0 || parts[k][0] + parts[k][1] > desc_bytes) return SSDHIP_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(desc_dev) | reinterpret_cast<uintptr_t>(coef_dev) | reinterpret_cast<uintptr_t>(planes_dev)) & 15)
        return SSDHIP_E_BADARG;
    if (indexed && (n_entries < 0 || ckpt_entries < 0 || (ckpt_entries > 0 && !ckpt_dev) || (reinterpret_cast<uintptr_t>(ckpt_dev) & 15) ||
                    record_segments < 0 || record_segments > n_segments || entry_lanes_per_wave < 1 || entry_lanes_per_wave > 64))
        return SSDHIP_E_BADARG;
    unsigned char* base = static_cast<unsigned char*>(desc_dev);
    JpegBatch b;
    b.images = reinterpret_cast<const ssdhip_jpeg_image*>(base + off_images);
    b.segments = reinterpret_cast<const ssdhip_jpeg_segment*>(base + off_segments);
    b.qt = reinterpret_cast<const unsigned short*>(base + off_qt);
    b.huff = reinterpret_cast<const ssdhip_jpeg_huff*>(base + off_huff);
    b.data = base + off_data;
    b.status = reinterpret_cast<int*>(base + off_status);
    b.n_images = n_images, b.n_segments = n_segments, b.n_qt = n_qt, b.n_huff = n_huff, b.data_bytes = data_bytes;
    b.total_blocks = total_blocks, b.out_bytes = out_bytes;
    if ((stages & 1) && !indexed) {
        const unsigned int groups = (unsigned int)((n_segments + lanes_per_wave - 1) / lanes_per_wave);
        hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(groups), dim3(64), 0, stream, b, lanes_per_wave, static_cast<short*>(coef_dev));
    }
    if ((stages & 1) && indexed) {
        JpegIndexArgs x;
        x.entries = reinterpret_cast<const ssdhip_jpeg_entry*>(base + off_entries);
        x.modes = reinterpret_cast<const int*>(base + off_modes);
        x.ckpt = static_cast<ssdhip_jpeg_entry*>(ckpt_dev);
        x.n_entries = n_entries, x.ckpt_entries = ckpt_entries;
        if (n_entries > 0) {
            const unsigned int groups = (unsigned int)((n_entries + entry_lanes_per_wave - 1) / entry_lanes_per_wave);
            hipLaunchKernelGGL(jpeg_entropy_entry_kernel, dim3(groups), dim3(64), 0, stream, b, x, entry_lanes_per_wave,
                               static_cast<short*>(coef_dev));
        }
        if (record_segments > 0) {                               // (0: every image has an index)
            const unsigned int groups = (unsigned int)((n_segments + lanes_per_wave - 1) / lanes_per_wave);
            hipLaunchKernelGGL(jpeg_entropy_record_kernel, dim3(groups), dim3(64), 0, stream, b, x, lanes_per_wave,
                               static_cast<short*>(coef_dev));
        }
    }
    if (stages & 2)
        hipLaunchKernelGGL(jpeg_block_kernel, dim3((unsigned int)((max_blocks + 255) / 256), (unsigned int)n_images), dim3(256), 0, stream,
                           b, static_cast<const short*>(coef_dev), static_cast<unsigned char*>(planes_dev));
    if (stages & 4)
        hipLaunchKernelGGL(jpeg_pixel_kernel, dim3((unsigned int)((max_pixels + 255) / 256), (unsigned int)n_images), dim3(256), 0, stream,
                           b, static_cast<const unsigned char*>(planes_dev), static_cast<unsigned char*>(out_dev));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

}  // namespace

extern "C" int ssdhip_jpeg_decode_batch(void* desc_dev, long long desc_bytes, int n_images, int n_segments, int n_qt, int n_huff,
                                        int off_images, int off_segments, int off_qt, int off_huff, int off_data, int data_bytes,
                                        int off_status, int max_blocks, int max_pixels, long long total_blocks, int lanes_per_wave,
                                        int stages, void* coef_dev, void* planes_dev, void* out_dev, long long out_bytes,
                                        void* stream_) {
    return jpeg_decode_batch(desc_dev, desc_bytes, n_images, n_segments, n_qt, n_huff, off_images, off_segments, off_qt, off_huff, off_data,
                             data_bytes, off_status, max_blocks, max_pixels, total_blocks, lanes_per_wave, stages, coef_dev, planes_dev,
                             out_dev, out_bytes, static_cast<hipStream_t>(stream_), false, 0, 0, 0, nullptr, 0, 0, 1);
}

extern "C" int ssdhip_jpeg_decode_batch_indexed(void* desc_dev, long long desc_bytes, int n_images, int n_segments, int n_qt, int n_huff,
                                                int off_images, int off_segments, int off_qt, int off_huff, int off_data, int data_bytes,
                                                int off_status, int off_entries, int n_entries, int off_modes, void* ckpt_dev,
                                                int ckpt_entries, int record_segments, int max_blocks, int max_pixels,
                                                long long total_blocks, int entry_lanes_per_wave, int lanes_per_wave, int stages,
                                                void* coef_dev, void* planes_dev, void* out_dev, long long out_bytes, void* stream_) {
    return jpeg_decode_batch(desc_dev, desc_bytes, n_images, n_segments, n_qt, n_huff, off_images, off_segments, off_qt, off_huff, off_data,
                             data_bytes, off_status, max_blocks, max_pixels, total_blocks, lanes_per_wave, stages, coef_dev, planes_dev,
                             out_dev, out_bytes, static_cast<hipStream_t>(stream_), true, off_entries, n_entries, off_modes, ckpt_dev,
                             ckpt_entries, record_segments, entry_lanes_per_wave);
}
