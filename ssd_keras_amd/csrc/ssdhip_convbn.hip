// ssdhip_convbn.hip -- SSD7's blocks, Conv2D(k, padding='same') -> BatchNormalization(axis=3, inference) -> ELU(alpha=1)
// [-> MaxPooling2D(2, 2) 'valid'] (reference models/keras_ssd7.py:277-309), as ONE launch each: gfx950, bf16 NHWC maps, float32
// accumulation on v_mfma_f32_32x32x16_bf16, plain C++ and the MFMA builtin only.
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

namespace ssdhip {
namespace {

constexpr int CBN_THREADS = 256;                         // four waves: wave i owns rows 2 i, 2 i + 1 of a tile
constexpr int CBN_TH = 8, CBN_TW = 32;                   // output tile
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

__device__ __forceinline__ void cbn_tile_origin(const CbnParams& p, int tile, int& b, int& h0, int& w0) {
    const int wt = tile % p.WT, q = tile / p.WT;
    b = q / p.HT;
    h0 = (q - b * p.HT) * CBN_TH;
    w0 = wt * CBN_TW;
}

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
// LDS: tables | filters [tap][NT 32 co][Cin + 8] | halo [10 x 34 pixels][Cin + 8].  The 16 bytes of padding behind every row of Cin
// values keep the fragment reads of 32 consecutive rows off one bank set; they are never read.
template <int CIN, int COUT>
struct Cbn3 {
    static constexpr int NT = (COUT + 31) / 32, PS = CIN * 2 + 16, KS = CIN / 16, CH = CIN / 8;
    static constexpr int HR = CBN_TH + 2, HC = CBN_TW + 2, HPX = HR * HC, NCHUNK = HPX * CH;
    static constexpr int NLD = (NCHUNK + CBN_THREADS - 1) / CBN_THREADS;
    static constexpr int WBYTES = 9 * NT * 32 * PS, LDS = CBN_TAB + WBYTES + HPX * PS;
    static_assert(LDS <= 160 * 1024 && CIN % 16 == 0, "LDS budget; whole MFMA steps");
};

template <int CIN, int COUT, bool POOL, int EPI>
__global__ __launch_bounds__(CBN_THREADS) void convbn3_kernel(const CbnParams p) {
    using G = Cbn3<CIN, COUT>;
    constexpr int NT = G::NT, PS = G::PS, KS = G::KS, CH = G::CH, HC = G::HC, NCHUNK = G::NCHUNK, NLD = G::NLD;
    extern __shared__ __attribute__((aligned(16))) unsigned char cbn_lds[];
    float* tab = reinterpret_cast<float*>(cbn_lds);
    unsigned char* wl = cbn_lds + CBN_TAB;
    unsigned char* hl = wl + G::WBYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r31 = lane & 31, khalf = lane >> 5;
    const int stride = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    if (tile >= p.tiles) return;

    // the 16-byte chunks of a tile's halo, dealt to the threads: chunk n = pixel n / CH (row hr, column hc), channels 8 (n % CH) ...
    auto fetch = [&](int t, u32x4 (&r)[NLD]) {
        int b, h0, w0;
        cbn_tile_origin(p, t, b, h0, w0);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int n = tid + CBN_THREADS * i, px = n / CH, c = n - px * CH, hr = px / HC, hc = px - hr * HC;
            const int h = h0 - 1 + hr, w = w0 - 1 + hc;
            r[i] = u32x4{0u, 0u, 0u, 0u};            // outside the image: the layer's zero padding
            if (n < NCHUNK && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W)
                r[i] = *reinterpret_cast<const u32x4*>(p.x + (((size_t)b * p.H + h) * p.W + w) * (CIN * 2) + c * 16);
        }
    };
    auto stash = [&](const u32x4 (&r)[NLD]) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int n = tid + CBN_THREADS * i, px = n / CH, c = n - px * CH;
            if (n < NCHUNK) *reinterpret_cast<u32x4*>(hl + px * PS + c * 16) = r[i];
        }
    };

    u32x4 raw[NLD];
    fetch(tile, raw);
    for (int i = tid; i < G::WBYTES / 16; i += CBN_THREADS)              // the resident filters: the packed image as it is
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
        cbn_tile_origin(p, tile, b, h0, w0);
        cbn_epilogue<COUT, POOL, EPI>(acc, tab, p, b, h0 + 2 * wave, w0 + r31, lane);
        __syncthreads();                                 // every wave is done with the halo before the next one overwrites it
    }
}

// ---- 5 x 5, Cin = 3, Cout = 32 ------------------------------------------------------------------------------------------------
// Halo: 12 rows x 36 pixels x 3 channels = 108 bf16 a row, in 224-byte LDS rows (the 8 bytes behind the data stay zero: the sixteenth
// k of the last columns and the aligned dword reads reach into them).  Packed filters: [kh][co][16] bf16, k = 3 kw + ci, k = 15 zero.
constexpr int CBN5_HR = CBN_TH + 4, CBN5_HC = CBN_TW + 4, CBN5_ROW = CBN5_HC * 3, CBN5_RS = 224, CBN5_NEL = CBN5_HR * CBN5_ROW;
constexpr int CBN5_NLD = (CBN5_NEL + CBN_THREADS - 1) / CBN_THREADS;

template <bool POOL, int EPI>
__global__ __launch_bounds__(CBN_THREADS) void convbn5_kernel(const CbnParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char cbn_lds[CBN_TAB + CBN5_HR * CBN5_RS];
    float* tab = reinterpret_cast<float*>(cbn_lds);
    unsigned char* hl = cbn_lds + CBN_TAB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r31 = lane & 31, khalf = lane >> 5;
    const int stride = (int)gridDim.x;
    int tile = (int)blockIdx.x;
    if (tile >= p.tiles) return;
    const unsigned short* x = reinterpret_cast<const unsigned short*>(p.x);

    auto fetch = [&](int t, unsigned short (&r)[CBN5_NLD]) {
        int b, h0, w0;
        cbn_tile_origin(p, t, b, h0, w0);
#pragma unroll
        for (int i = 0; i < CBN5_NLD; ++i) {
            const int n = tid + CBN_THREADS * i, hr = n / CBN5_ROW, e = n - hr * CBN5_ROW, hc = e / 3;
            const int h = h0 - 2 + hr, w = w0 - 2 + hc;
            r[i] = 0;
            if (n < CBN5_NEL && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W)
                r[i] = x[(((size_t)b * p.H + h) * p.W + w) * 3 + (e - hc * 3)];
        }
    };
    auto stash = [&](const unsigned short (&r)[CBN5_NLD]) {
#pragma unroll
        for (int i = 0; i < CBN5_NLD; ++i) {
            const int n = tid + CBN_THREADS * i, hr = n / CBN5_ROW, e = n - hr * CBN5_ROW;
            if (n < CBN5_NEL) *reinterpret_cast<unsigned short*>(hl + hr * CBN5_RS + e * 2) = r[i];
        }
    };

    unsigned short raw[CBN5_NLD];
    fetch(tile, raw);
    bf16x8 a[5];
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) a[kh] = *reinterpret_cast<const bf16x8*>(p.w + ((kh * 32 + r31) * 16 + khalf * 8) * 2);
    cbn_load_tables<EPI>(tab, p, 32, tid);
    if (tid < CBN5_HR * 2) *reinterpret_cast<unsigned*>(hl + (tid >> 1) * CBN5_RS + CBN5_ROW * 2 + (tid & 1) * 4) = 0u;

    // the lane's operand of kernel row kh: 16 bytes at 6 bytes a column, i.e. on a half-dword boundary for odd columns -- five aligned
    // dwords, shifted by two bytes where needed; the sixteenth k (the next pixel's first channel) is cleared, its filter value is zero
    const unsigned off = (unsigned)(r31 * 6 + khalf * 16);
    const unsigned char* bptr = hl + (2 * wave) * CBN5_RS + (off & ~3u);
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
                const unsigned* q = reinterpret_cast<const unsigned*>(bptr + (r + kh) * CBN5_RS);
                const unsigned d[5] = {q[0], q[1], q[2], q[3], q[4]};
                u32x4 f;
#pragma unroll
                for (int i = 0; i < 4; ++i) f[i] = (unsigned)(((((unsigned long long)d[i + 1]) << 32) | d[i]) >> shift);
                f[3] &= last;
                acc[r][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kh], __builtin_bit_cast(bf16x8, f), acc[r][0], 0, 0, 0);
            }
        int b, h0, w0;
        cbn_tile_origin(p, tile, b, h0, w0);
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

template <int CIN, int COUT, bool POOL, int EPI = CBN_BN_ELU>
int cbn_launch3(const CbnParams& p, hipStream_t stream) {
    using G = Cbn3<CIN, COUT>;
    auto fn = convbn3_kernel<CIN, COUT, POOL, EPI>;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS);
    if (attr != hipSuccess) return SSDHIP_E_LAUNCH;
    int per_cu = (160 * 1024) / G::LDS;                  // workgroups that fit a CU's LDS; two keep a CU busy across the barriers
    per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
    const long long cap = (long long)cbn_cu_count() * per_cu;
    const int grid = (int)(p.tiles < cap ? p.tiles : cap);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(CBN_THREADS), G::LDS, stream, p);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

template <int CIN, int COUT>
int cbn_launch3(const CbnParams& p, int pool, hipStream_t stream) {
    return pool ? cbn_launch3<CIN, COUT, true>(p, stream) : cbn_launch3<CIN, COUT, false>(p, stream);
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

// elements of the image of a (rows = Cout, cols = Cin) 3 x 3 layer
__host__ __device__ inline int cbn_image3_elems(int cin, int cout) { return 9 * ((cout + 31) / 32) * 32 * (cin + 8); }

__global__ __launch_bounds__(256) void cbn_pack_kernel(const CbnPackTable t) {
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
    const int rows = flip ? L.cin : L.cout, cols = flip ? L.cout : L.cin, rp = (rows + 31) / 32 * 32, cp = cols + 8;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < 9 * rp * cp; i += step) {
        const int c = i % cp, q = i / cp, r = q % rp, tap = q / rp, kh = tap / 3, kw = tap - 3 * kh;
        bf16_t v = 0;
        if (r < rows && c < cols)
            v = flip ? L.w[c * L.s[0] + r * L.s[1] + (2 - kh) * L.s[2] + (2 - kw) * L.s[3]] : L.w[r * L.s[0] + c * L.s[1] + kh * L.s[2] + kw * L.s[3]];
        out[i] = v;
    }
}

}  // namespace
}  // namespace ssdhip

using namespace ssdhip;

extern "C" size_t ssdhip_conv_bn_elu_pack_bytes(int Cin, int Cout, int kernel) {
    if (kernel == 5 && Cin == 3 && Cout == 32) return 5 * 32 * 16 * 2;
    if (kernel != 3) return 0;
    const bool ok = (Cin == 32 && Cout == 48) || (Cin == 48 && (Cout == 64 || Cout == 48 || Cout == 32)) || (Cin == 64 && (Cout == 64 || Cout == 48));
    return ok ? (size_t)9 * ((Cout + 31) / 32) * 32 * (Cin * 2 + 16) : 0;
}

namespace ssdhip {
namespace {
// Both epilogues: the checks every launch shares, then the geometry's instantiation (scale / shift: CBN_BN_ELU; bias: CBN_BIAS).
int cbn_run(int epi, const void* x, const void* w_packed, const float* scale, const float* shift, const void* bias, void* y, int B, int H, int W,
            int Cin, int Cout, int kernel, int pool, hipStream_t stream) {
    if (!x || !w_packed || !y || B <= 0 || H <= 0 || W <= 0) return SSDHIP_E_BADARG;
    if (epi == CBN_BN_ELU && (!scale || !shift)) return SSDHIP_E_BADARG;
    if (ssdhip_conv_bn_elu_pack_bytes(Cin, Cout, kernel) == 0) return SSDHIP_E_BADARG;
    if (pool && (H < 2 || W < 2)) return SSDHIP_E_BADARG;
    if ((((uintptr_t)w_packed | (uintptr_t)y) & 15) || ((uintptr_t)x & (kernel == 3 ? 15 : 1)) || (((uintptr_t)scale | (uintptr_t)shift) & 3) ||
        ((uintptr_t)bias & 1))
        return SSDHIP_E_BADARG;
    CbnParams p;
    p.x = static_cast<const unsigned char*>(x); p.w = static_cast<const unsigned char*>(w_packed);
    p.scale = scale; p.shift = shift; p.bias = static_cast<const bf16_t*>(bias); p.y = static_cast<unsigned char*>(y);
    p.B = B; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
    p.HT = (H + CBN_TH - 1) / CBN_TH; p.WT = (W + CBN_TW - 1) / CBN_TW;
    const long long tiles = (long long)B * p.HT * p.WT;
    if (tiles > 0x3fffffffLL || (long long)B * H * W > 0x3fffffffLL) return SSDHIP_E_BADARG;
    p.tiles = (int)tiles;
    if (kernel == 5) {
        const long long cap = (long long)cbn_cu_count() * 4;
        const int grid = (int)(tiles < cap ? tiles : cap);
        if (epi == CBN_BIAS) hipLaunchKernelGGL((convbn5_kernel<false, CBN_BIAS>), dim3(grid), dim3(CBN_THREADS), 0, stream, p);
        else if (pool) hipLaunchKernelGGL((convbn5_kernel<true, CBN_BN_ELU>), dim3(grid), dim3(CBN_THREADS), 0, stream, p);
        else hipLaunchKernelGGL((convbn5_kernel<false, CBN_BN_ELU>), dim3(grid), dim3(CBN_THREADS), 0, stream, p);
        return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
    }
    if (epi == CBN_BIAS) {
        if (Cin == 32) return cbn_launch3<32, 48, false, CBN_BIAS>(p, stream);
        if (Cin == 48)
            return Cout == 64 ? cbn_launch3<48, 64, false, CBN_BIAS>(p, stream)
                              : Cout == 48 ? cbn_launch3<48, 48, false, CBN_BIAS>(p, stream) : cbn_launch3<48, 32, false, CBN_BIAS>(p, stream);
        return Cout == 64 ? cbn_launch3<64, 64, false, CBN_BIAS>(p, stream) : cbn_launch3<64, 48, false, CBN_BIAS>(p, stream);
    }
    if (Cin == 32) return cbn_launch3<32, 48>(p, pool, stream);
    if (Cin == 48) return Cout == 64 ? cbn_launch3<48, 64>(p, pool, stream) : Cout == 48 ? cbn_launch3<48, 48>(p, pool, stream) : cbn_launch3<48, 32>(p, pool, stream);
    return Cout == 64 ? cbn_launch3<64, 64>(p, pool, stream) : cbn_launch3<64, 48>(p, pool, stream);
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
        if (!weights[i] || !fwd[i] || ssdhip_conv_bn_elu_pack_bytes(Cin[i], Cout[i], kernel[i]) == 0) return SSDHIP_E_BADARG;
        if (kernel[i] == 5 && flipped[i]) return SSDHIP_E_BADARG;       // the first layer has no data gradient
        if (((uintptr_t)weights[i] | (uintptr_t)fwd[i] | (uintptr_t)flipped[i]) & 1) return SSDHIP_E_BADARG;
        long long reach = 0;                              // the farthest element the strides address: a sanity bound, not the tensor's size
        const int dims[4] = {Cout[i], Cin[i], kernel[i], kernel[i]};
        for (int d = 0; d < 4; ++d) {
            if (strides[4 * i + d] < 0) return SSDHIP_E_BADARG;
            reach += strides[4 * i + d] * (dims[d] - 1);
            L.s[d] = strides[4 * i + d];
        }
        if (reach > 0x3fffffffLL) return SSDHIP_E_BADARG;
        L.w = static_cast<const bf16_t*>(weights[i]); L.fwd = static_cast<bf16_t*>(fwd[i]); L.flip = static_cast<bf16_t*>(flipped[i]);
        L.cin = Cin[i]; L.cout = Cout[i]; L.kernel = kernel[i];
        const int n = kernel[i] == 5 ? 5 * 32 * 16 : cbn_image3_elems(Cin[i] > Cout[i] ? Cin[i] : Cout[i], Cin[i] > Cout[i] ? Cin[i] : Cout[i]);
        most = n > most ? n : most;
    }
    const int bx = (most + 256 * 4 - 1) / (256 * 4);      // about four elements a thread in the largest image
    hipLaunchKernelGGL(cbn_pack_kernel, dim3(bx, 2 * n_layers), dim3(256), 0, static_cast<hipStream_t>(stream_), t);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
