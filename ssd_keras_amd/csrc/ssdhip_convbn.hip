// ssdhip_convbn.hip -- SSD7's blocks, Conv2D(k, padding='same') -> BatchNormalization(axis=3, inference) -> ELU(alpha=1)
// [-> MaxPooling2D(2, 2) 'valid'] (reference models/keras_ssd7.py:277-309), as ONE launch each: gfx950, bf16 NHWC maps, float32
// accumulation on v_mfma_f32_32x32x16_bf16, plain C++ and the MFMA builtin only.
//
// What this file shares with the weight-gradient files (geometries, tile grid, halo layouts, launch helper) is in ssdhip_ssd7.h.
//
// Geometries (exactly SSD7's; anything else is SSDHIP_E_BADARG):
//   * 3 x 3, stride 1, pad 1, (Cin, Cout) in {(32, 48), (48, 64), (64, 64), (64, 48), (48, 48), (48, 32)}: K = 9 Cin, taps outer,
//     channels inner.  Cout = 48 runs as two 32-column tiles whose last 16 filter rows are zero and whose lanes store nothing.
//   * 5 x 5, stride 1, pad 2, Cin = 3, Cout = 32: the 15 values of a kernel row (k = 3 kw + ci) are 15 CONSECUTIVE bf16 of the
//     image row, padded to 16 with a zero: K = 80 in five MFMA steps, the operand of a pixel is read from the halo at 6 bytes a column.
//
// Structure.  Persistent workgroups of four waves walk 8-row x 32-column output tiles.  The layer's whole filter set (at most 81 KB
// with its row padding) is copied into LDS once per workgroup (the 5 KB of the 5 x 5 layer live in registers); per tile only the
// (8 + k - 1) x (32 + k - 1)-pixel input halo comes in, through registers: the NEXT tile's halo is requested before the current
// tile's MFMAs and stored into LDS behind them, so the global latency is covered by the multiplication.  The taps are LDS
// displacements into the halo.  Zero padding -- at the map border and between images -- is written by the loader (a halo pixel
// outside its own image is stored as zeros; nothing is ever read from a neighbouring image and nothing relies on a memset).
// Each wave owns two rows x 32 columns, i.e. the two rows of 16 pooling windows, for all output channels.
//
// Epilogue = the numerical contract (tests/test_conv_bn_elu_gpu.py):  v = fmaf(acc, scale[c], shift[c]) in float32 (the tables are
// built by the caller in float64: scale = gamma / sqrt(var + eps), shift = beta + (conv_bias - mean) scale; no other bias);
// e = v > 0 ? v : expm1f(v);  with pool the maximum of the window's four e (BatchNorm and ELU FIRST: gamma may be negative, so the
// accumulators cannot be pooled);  one round-to-nearest-even conversion to bf16.
// In the accumulator layout a lane holds one pixel column and 4-channel runs: vertical maximum in the lane, horizontal with the
// neighbouring lane, 8-byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_bf16.h"
#include "ssdhip_ssd7.h"

namespace ssdhip {
namespace {

// Four waves (S7_THREADS) on an S7_TH x S7_TW output tile: wave i owns rows 2 i, 2 i + 1.
constexpr int CBN_TAB = 512;                             // LDS: scale[64] | shift[64] float32
// Epilogue modes.  CBN_BN_ELU: the block of the inference path (below).  CBN_BIAS: the plain convolution of the TRAINING step and its
// data gradient -- y = bf16(acc + float(bias[c])), one float32 add and one rounding, full-size map only; the bias is the layer's own
// bf16 parameter, widened here (tab[c]; zeros for a NULL bias, which is what the data gradient passes).
constexpr int CBN_BN_ELU = 0, CBN_BIAS = 1;

struct CbnParams {
    const unsigned char* x;      // [B, H, W, Cin] bf16
    const unsigned char* w;      // packed filters (ssdhip_conv_bn_elu_pack_bytes)
    const float* scale;          // [Cout]
    const float* shift;          // [Cout]
    const bf16_t* bias;          // CBN_BIAS: [Cout] bf16 or NULL (no bias)
    unsigned char* y;            // [B, H, W, Cout] or pooled [B, H / 2, W / 2, Cout] bf16
    int B, H, W, Ho, Wo;
    int HT, WT, tiles;           // tile grid per image, tiles = B HT WT
};

__device__ __forceinline__ float cbn_max(float a, float b) { return (a > b || a != a) ? a : b; }    // NaN wins, as in max_pool2d

// acc[r][nt]: rows h, h + 1 of image b, column w = the lane's (lane & 31), channel (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of tile nt.
template <int COUT, bool POOL, int EPI>
__device__ __forceinline__ void cbn_epilogue(const f32x16 (&acc)[2][(COUT + 31) / 32], const float* tab, const CbnParams& p, int b, int h,
                                             int w, int lane) {
    constexpr int NT = (COUT + 31) / 32;
    const int khalf = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (nt * 32 + 8 * g >= COUT) continue;       // the zero filter rows of a 48-channel layer's second tile
            const int c = nt * 32 + 8 * g + 4 * khalf;
            const float4 sc = *reinterpret_cast<const float4*>(tab + c), sh = *reinterpret_cast<const float4*>(tab + 64 + c);
            const float s[4] = {sc.x, sc.y, sc.z, sc.w}, t[4] = {sh.x, sh.y, sh.z, sh.w};
            float e[2][4];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (EPI == CBN_BIAS) {
                        e[r][i] = acc[r][nt][4 * g + i] + s[i];
                    } else {
                        const float v = fmaf(acc[r][nt][4 * g + i], s[i], t[i]);
                        e[r][i] = v > 0.f ? v : expm1f(v);
                    }
                }
            if constexpr (POOL) {
                float m[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    m[i] = cbn_max(e[0][i], e[1][i]);
                    m[i] = cbn_max(m[i], __shfl_xor(m[i], 1));
                }
                const int ph = h >> 1, pw = w >> 1;
                if (!(lane & 1) && ph < p.Ho && pw < p.Wo)
                    *reinterpret_cast<uint2*>(p.y + (((size_t)b * p.Ho + ph) * p.Wo + pw) * (COUT * 2) + c * 2) =
                        make_uint2(pack2_bf16(m[0], m[1]), pack2_bf16(m[2], m[3]));
            } else {
#pragma unroll
                for (int r = 0; r < 2; ++r)
                    if (h + r < p.H && w < p.W)
                        *reinterpret_cast<uint2*>(p.y + (((size_t)b * p.H + h + r) * p.W + w) * (COUT * 2) + c * 2) =
                            make_uint2(pack2_bf16(e[r][0], e[r][1]), pack2_bf16(e[r][2], e[r][3]));
            }
        }
}

template <int EPI>
__device__ __forceinline__ void cbn_load_tables(float* tab, const CbnParams& p, int cout, int tid) {
    if (tid < 64) {
        if constexpr (EPI == CBN_BIAS) {
            tab[tid] = (tid < cout && p.bias) ? bf16_float(p.bias[tid]) : 0.f;
            tab[64 + tid] = 0.f;
        } else {
            tab[tid] = tid < cout ? p.scale[tid] : 0.f;
            tab[64 + tid] = tid < cout ? p.shift[tid] : 0.f;
        }
    }
}

// ---- 3 x 3 ------------------------------------------------------------------------------------------------------------------------
// LDS: tables | filters [tap][NT 32 co][Cin + 8] | halo [10 x 34 pixels][Cin + 8] (S7Halo3).  The 16 bytes of padding behind every row
// of Cin values keep the fragment reads of 32 consecutive rows off one bank set; they are never read.
template <int CIN, int COUT>
struct Cbn3 {
    using Halo = S7Halo3<CIN>;
    static constexpr int NT = (COUT + 31) / 32, PS = Halo::PS, KS = CIN / 16;
    static constexpr int WBYTES = 9 * NT * 32 * PS, LDS = CBN_TAB + WBYTES + Halo::BYTES;
    static_assert(LDS <= 160 * 1024 && CIN % 16 == 0, "LDS budget; whole MFMA steps");
};

template <int CIN, int COUT, bool POOL, int EPI>
__global__ __launch_bounds__(S7_THREADS) void convbn3_kernel(const CbnParams p) {
    using G = Cbn3<CIN, COUT>;
    using Halo = typename G::Halo;
    constexpr int NT = G::NT, PS = G::PS, KS = G::KS, CH = Halo::CH, HC = Halo::HC, NCHUNK = Halo::NCHUNK, NLD = Halo::NLD;
    extern __shared__ __attribute__((aligned(16))) unsigned char cbn_lds[];
    float* tab = reinterpret_cast<float*>(cbn_lds);
    unsigned char* wl = cbn_lds + CBN_TAB;
    unsigned char* hl = wl + G::WBYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r31 = lane & 31, khalf = lane >> 5;
    const int stride = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    if (tile >= p.tiles) return;

    // the 16-byte chunks of a tile's halo (S7Halo3), dealt to the threads: chunk n = pixel n / CH (row hr, column hc), channels 8 (n % CH) ...
    auto fetch = [&](int t, u32x4 (&r)[NLD]) {
        int b, h0, w0;
        ssd7_tile_origin(p, t, b, h0, w0);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int n = tid + S7_THREADS * i, px = n / CH, c = n - px * CH, hr = px / HC, hc = px - hr * HC;
            const int h = h0 - 1 + hr, w = w0 - 1 + hc;
            r[i] = u32x4{0u, 0u, 0u, 0u};            // outside the image: the layer's zero padding
            if (n < NCHUNK && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W)
                r[i] = *reinterpret_cast<const u32x4*>(p.x + (((size_t)b * p.H + h) * p.W + w) * (CIN * 2) + c * 16);
        }
    };
    auto stash = [&](const u32x4 (&r)[NLD]) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int n = tid + S7_THREADS * i, px = n / CH, c = n - px * CH;
            if (n < NCHUNK) *reinterpret_cast<u32x4*>(hl + px * PS + c * 16) = r[i];
        }
    };

    u32x4 raw[NLD];
    fetch(tile, raw);
    for (int i = tid; i < G::WBYTES / 16; i += S7_THREADS)              // the resident filters: the packed image as it is
        reinterpret_cast<u32x4*>(wl)[i] = reinterpret_cast<const u32x4*>(p.w)[i];
    cbn_load_tables<EPI>(tab, p, COUT, tid);

    const unsigned char* bptr = hl + ((2 * wave) * HC + r31) * PS + khalf * 16;
    const unsigned char* aptr = wl + r31 * PS + khalf * 16;
    for (; tile < p.tiles; tile += stride) {
        stash(raw);
        __syncthreads();                                 // this tile's halo (first pass: filters and tables too) is in LDS
        if (tile + stride < p.tiles) fetch(tile + stride, raw);          // in flight during the MFMAs

        f32x16 acc[2][NT];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[r][nt][v] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int boff = ((t / 3) * HC + (t % 3)) * PS + kk * 32;
                const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(bptr + boff);
                const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(bptr + boff + HC * PS);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(aptr + (t * NT + nt) * 32 * PS + kk * 32);
                    acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0, acc[0][nt], 0, 0, 0);
                    acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b1, acc[1][nt], 0, 0, 0);
                }
            }
        int b, h0, w0;
        ssd7_tile_origin(p, tile, b, h0, w0);
        cbn_epilogue<COUT, POOL, EPI>(acc, tab, p, b, h0 + 2 * wave, w0 + r31, lane);
        __syncthreads();                                 // every wave is done with the halo before the next one overwrites it
    }
}

// ---- 5 x 5, Cin = 3, Cout = 32 ------------------------------------------------------------------------------------------------
// Halo: S7Halo5 (the 8 bytes behind a row's data stay zero: the sixteenth k of the last columns and the aligned dword reads reach into
// them).  Packed filters: [kh][co][16] bf16, k = 3 kw + ci, k = 15 zero.

template <bool POOL, int EPI>
__global__ __launch_bounds__(S7_THREADS) void convbn5_kernel(const CbnParams p) {
    using Halo = S7Halo5;
    __shared__ __attribute__((aligned(16))) unsigned char cbn_lds[CBN_TAB + Halo::BYTES];
    float* tab = reinterpret_cast<float*>(cbn_lds);
    unsigned char* hl = cbn_lds + CBN_TAB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r31 = lane & 31, khalf = lane >> 5;
    const int stride = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    if (tile >= p.tiles) return;

    const unsigned short* x = reinterpret_cast<const unsigned short*>(p.x);

    auto fetch = [&](int t, unsigned short (&r)[Halo::NLD]) {
        int b, h0, w0;
        ssd7_tile_origin(p, t, b, h0, w0);
#pragma unroll
        for (int i = 0; i < Halo::NLD; ++i) {
            const int n = tid + S7_THREADS * i, hr = n / Halo::ROW, e = n - hr * Halo::ROW, hc = e / 3;
            const int h = h0 - 2 + hr, w = w0 - 2 + hc;
            r[i] = 0;
            if (n < Halo::NEL && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W)
                r[i] = x[(((size_t)b * p.H + h) * p.W + w) * 3 + (e - hc * 3)];
        }
    };
    auto stash = [&](const unsigned short (&r)[Halo::NLD]) {
#pragma unroll
        for (int i = 0; i < Halo::NLD; ++i) {
            const int n = tid + S7_THREADS * i, hr = n / Halo::ROW, e = n - hr * Halo::ROW;
            if (n < Halo::NEL) *reinterpret_cast<unsigned short*>(hl + hr * Halo::RS + e * 2) = r[i];
        }
    };

    unsigned short raw[Halo::NLD];
    fetch(tile, raw);
    bf16x8 a[5];
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) a[kh] = *reinterpret_cast<const bf16x8*>(p.w + ((kh * 32 + r31) * 16 + khalf * 8) * 2);
    cbn_load_tables<EPI>(tab, p, 32, tid);
    if (tid < Halo::HR * 2) *reinterpret_cast<unsigned*>(hl + (tid >> 1) * Halo::RS + Halo::ROW * 2 + (tid & 1) * 4) = 0u;

    // the lane's operand of kernel row kh: 16 bytes at 6 bytes a column, i.e. on a half-dword boundary for odd columns -- five aligned
    // dwords, shifted by two bytes where needed; the sixteenth k (the next pixel's first channel) is cleared, its filter value is zero
    const unsigned off = (unsigned)(r31 * 6 + khalf * 16);
    const unsigned char* bptr = hl + (2 * wave) * Halo::RS + (off & ~3u);
    const unsigned shift = (off & 2u) * 8u, last = khalf ? 0x0000ffffu : 0xffffffffu;
    for (; tile < p.tiles; tile += stride) {
        stash(raw);
        __syncthreads();
        if (tile + stride < p.tiles) fetch(tile + stride, raw);

        f32x16 acc[2][1];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[r][0][v] = 0.f;
#pragma unroll
        for (int kh = 0; kh < 5; ++kh)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const unsigned* q = reinterpret_cast<const unsigned*>(bptr + (r + kh) * Halo::RS);
                const unsigned d[5] = {q[0], q[1], q[2], q[3], q[4]};
                u32x4 f;
#pragma unroll
                for (int i = 0; i < 4; ++i) f[i] = (unsigned)(((((unsigned long long)d[i + 1]) << 32) | d[i]) >> shift);
                f[3] &= last;
                acc[r][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kh], __builtin_bit_cast(bf16x8, f), acc[r][0], 0, 0, 0);
            }
        int b, h0, w0;
        ssd7_tile_origin(p, tile, b, h0, w0);
        cbn_epilogue<32, POOL, EPI>(acc, tab, p, b, h0 + 2 * wave, w0 + r31, lane);
        __syncthreads();
    }
}

int cbn_cu_count() {
    static const int n = []() {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            return 256;
        return cus;
    }();
    return n;
}

// The geometry's instantiation of one epilogue.  3 x 3: as many workgroups as fit the CUs' LDS, at most two a CU (two keep a CU busy
// across the barriers); 5 x 5: four a CU.
template <bool POOL, int EPI>
int cbn_launch(const CbnParams& p, int Cin, int Cout, int kernel, hipStream_t stream) {
    if (kernel == 5) {
        const long long cap = (long long)cbn_cu_count() * 4;
        return ssd7_launch<convbn5_kernel<POOL, EPI>>(dim3((int)(p.tiles < cap ? p.tiles : cap)), 0, 0, stream, p);
    }
    int rc = SSDHIP_E_BADARG;
    ssd7_for_pair3(Cin, Cout, [&](auto ci, auto co) {
        constexpr int CIN = decltype(ci)::value, COUT = decltype(co)::value, LDS = Cbn3<CIN, COUT>::LDS;
        int per_cu = (160 * 1024) / LDS;
        per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
        const long long cap = (long long)cbn_cu_count() * per_cu;
        rc = ssd7_launch<convbn3_kernel<CIN, COUT, POOL, EPI>>(dim3((int)(p.tiles < cap ? p.tiles : cap)), LDS, LDS, stream, p);
    });
    return rc;
}

// ---- filter images, refreshed on the device ----------------------------------------------------------------------------------------
// One launch writes EVERY byte of every image of a table of layers (padding rows and columns included: nothing relies on an earlier
// fill) from the bf16 parameters, read through their four element strides: the forward image of ssdhip_conv_bn_elu_pack_bytes and, for
// the 3 x 3 layers, the image of the data gradient's filters, w.flip(2, 3).transpose(0, 1) -- (Cin, Cout) swapped, taps flipped.
constexpr int CBN_PACK_MAX = 8;
struct CbnPackLayer {
    const bf16_t* w;
    bf16_t* fwd;
    bf16_t* flip;                // NULL: not wanted (always for the 5 x 5 layer, which has no data gradient)
    long long s[4];              // element strides of (Cout, Cin, kh, kw)
    int cin, cout, kernel;
};
struct CbnPackTable {
    CbnPackLayer layer[CBN_PACK_MAX];
};

__global__ __launch_bounds__(S7_THREADS) void cbn_pack_kernel(const CbnPackTable t) {
    const CbnPackLayer& L = t.layer[blockIdx.y >> 1];
    const bool flip = blockIdx.y & 1;
    bf16_t* out = flip ? L.flip : L.fwd;
    if (!out || !L.w) return;
    const int step = (int)(gridDim.x * blockDim.x);
    if (L.kernel == 5) {                                 // [kh][32][16], k = 3 kw + ci, k = 15 zero
        for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < 5 * 32 * 16; i += step) {
            const int k = i & 15, co = (i >> 4) & 31, kh = i >> 9;
            out[i] = k < 15 ? L.w[co * L.s[0] + (k % 3) * L.s[1] + kh * L.s[2] + (k / 3) * L.s[3]] : (bf16_t)0;
        }
        return;
    }
    // the image's rows / columns: forward (Cout, Cin); flipped (Cin, Cout), element (kh, kw, r, c) = w[c][r][2 - kh][2 - kw]
    ssd7_write_image3(out, flip ? L.cin : L.cout, flip ? L.cout : L.cin, (int)(blockIdx.x * blockDim.x + threadIdx.x), step,
                      [&](int r, int c, int kh, int kw) {
                          return flip ? L.w[c * L.s[0] + r * L.s[1] + (2 - kh) * L.s[2] + (2 - kw) * L.s[3]]
                                      : L.w[r * L.s[0] + c * L.s[1] + kh * L.s[2] + kw * L.s[3]];
                      });
}

}  // namespace
}  // namespace ssdhip

using namespace ssdhip;

extern "C" size_t ssdhip_conv_bn_elu_pack_bytes(int Cin, int Cout, int kernel) {
    if (!ssd7_geometry(Cin, Cout, kernel)) return 0;
    return kernel == 5 ? 5 * 32 * 16 * 2 : (size_t)ssd7_image3_elems(Cout, Cin) * 2;
}

namespace ssdhip {
namespace {
// Both epilogues: the checks every launch shares, then the geometry's instantiation (scale / shift: CBN_BN_ELU; bias: CBN_BIAS).
int cbn_run(int epi, const void* x, const void* w_packed, const float* scale, const float* shift, const void* bias, void* y, int B, int H, int W,
            int Cin, int Cout, int kernel, int pool, hipStream_t stream) {
    if (!x || !w_packed || !y || !ssd7_geometry(Cin, Cout, kernel)) return SSDHIP_E_BADARG;
    if (epi == CBN_BN_ELU && (!scale || !shift)) return SSDHIP_E_BADARG;
    if (pool && (H < 2 || W < 2)) return SSDHIP_E_BADARG;
    if ((((uintptr_t)w_packed | (uintptr_t)y) & 15) || ((uintptr_t)x & (kernel == 3 ? 15 : 1)) || (((uintptr_t)scale | (uintptr_t)shift) & 3) ||
        ((uintptr_t)bias & 1))
        return SSDHIP_E_BADARG;
    CbnParams p;
    if (!ssd7_tile_grid(B, H, W, p)) return SSDHIP_E_BADARG;
    p.x = static_cast<const unsigned char*>(x); p.w = static_cast<const unsigned char*>(w_packed);
    p.scale = scale; p.shift = shift; p.bias = static_cast<const bf16_t*>(bias); p.y = static_cast<unsigned char*>(y);
    p.Ho = H / 2; p.Wo = W / 2;
    if (epi == CBN_BIAS) return cbn_launch<false, CBN_BIAS>(p, Cin, Cout, kernel, stream);
    return pool ? cbn_launch<true, CBN_BN_ELU>(p, Cin, Cout, kernel, stream) : cbn_launch<false, CBN_BN_ELU>(p, Cin, Cout, kernel, stream);
}
}  // namespace
}  // namespace ssdhip

extern "C" int ssdhip_conv_bn_elu_nhwc_bf16(const void* x, const void* w_packed, const float* scale, const float* shift, void* y, int B, int H,
                                            int W, int Cin, int Cout, int kernel, int pool, void* stream_) {
    return cbn_run(CBN_BN_ELU, x, w_packed, scale, shift, nullptr, y, B, H, W, Cin, Cout, kernel, pool, static_cast<hipStream_t>(stream_));
}

extern "C" int ssdhip_conv_same_bias_nhwc_bf16(const void* x, const void* w_packed, const void* bias, void* y, int B, int H, int W, int Cin,
                                               int Cout, int kernel, void* stream_) {
    return cbn_run(CBN_BIAS, x, w_packed, nullptr, nullptr, bias, y, B, H, W, Cin, Cout, kernel, 0, static_cast<hipStream_t>(stream_));
}

extern "C" int ssdhip_ssd7_pack_filters(int n_layers, const void* const* weights, void* const* fwd, void* const* flipped, const int* Cin,
                                        const int* Cout, const int* kernel, const long long* strides, void* stream_) {
    if (n_layers <= 0 || n_layers > CBN_PACK_MAX || !weights || !fwd || !flipped || !Cin || !Cout || !kernel || !strides) return SSDHIP_E_BADARG;
    CbnPackTable t = {};
    int most = 0;
    for (int i = 0; i < n_layers; ++i) {
        CbnPackLayer& L = t.layer[i];
        if (!weights[i] || !fwd[i] || !ssd7_geometry(Cin[i], Cout[i], kernel[i])) return SSDHIP_E_BADARG;
        if (kernel[i] == 5 && flipped[i]) return SSDHIP_E_BADARG;       // the first layer has no data gradient
        if (((uintptr_t)weights[i] | (uintptr_t)fwd[i] | (uintptr_t)flipped[i]) & 1) return SSDHIP_E_BADARG;
        if (!ssd7_strides(strides + 4 * i, Cout[i], Cin[i], kernel[i], L.s)) return SSDHIP_E_BADARG;
        L.w = static_cast<const bf16_t*>(weights[i]); L.fwd = static_cast<bf16_t*>(fwd[i]); L.flip = static_cast<bf16_t*>(flipped[i]);
        L.cin = Cin[i]; L.cout = Cout[i]; L.kernel = kernel[i];
        const int side = Cin[i] > Cout[i] ? Cin[i] : Cout[i], n = kernel[i] == 5 ? 5 * 32 * 16 : ssd7_image3_elems(side, side);
        most = n > most ? n : most;
    }
    const int bx = (most + S7_THREADS * 4 - 1) / (S7_THREADS * 4);      // about four elements a thread in the largest image
    return ssd7_launch<cbn_pack_kernel>(dim3(bx, 2 * n_layers), 0, 0, static_cast<hipStream_t>(stream_), t);
}
