// ssdhip_wgrad7.hip -- weight and bias gradient of SSD7's seven trunk convolutions (reference models/keras_ssd7.py:277-309, the layers
// ssd7_training.ipynb trains), gfx950, bf16 NHWC operands, float32 accumulation on v_mfma_f32_32x32x16_bf16.
//
//     dw[co][kh][kw][ci] = sum_{b,h,w} dy[b,h,w,co] x[b, h + kh - p, w + kw - p, ci]        db[co] = sum_{b,h,w} dy[b,h,w,co]
//
// Geometries (exactly SSD7's; anything else is SSDHIP_E_BADARG and a workspace of 0 bytes): k = 3, p = 1 with (Cin, Cout) in {(32, 48),
// (48, 64), (64, 64), (64, 48), (48, 48), (48, 32)}; k = 5, p = 2 with (3, 32).
//
// The contraction runs over the pixels, the slow index of both NHWC operands (ssdhip_wgrad.hip has the long story).  Here:
//   * Cout <= 64 and k k Cin <= 576, so ONE workgroup holds a layer's whole [Cout][k k Cin] float32 tile in accumulators: four waves,
//     each a 32 x 32 (output channels x input channels) block for all nine taps -- or, where the layer has only two such blocks, for
//     five / four of the taps.  A persistent workgroup walks its share of the 8 x 32 position tiles of the forward kernel
//     (ssdhip_convbn.hip) on that kernel's halo layout (ssdhip_ssd7.h): the NEXT tile's halo and dy tile are requested before the current tile's
//     MFMAs and stored into LDS behind them.  Zero padding -- at the map border, between images and in the columns / rows of a partial
//     tile -- is written by the loader (dy is zero outside its image, so the finite x values beside a partial tile add nothing); no memset.
//   * both operands sit in LDS as [position][channels] images and are read with ds_read_b64_tr_b16: a lane gets four consecutive
//     positions of ITS channel.  That read wants all 64 lanes active and 8-byte-aligned lane addresses, so 48 channels run as two
//     32-channel blocks whose upper 16 lanes read whatever lies behind the pixel's values (inside the LDS allocation): padded, not
//     masked.  An MFMA output depends on its own row of A and column of B only, so those lanes' results -- never stored -- are the only
//     ones that see the padding.  A tap is a displacement of the per-lane row address; a K-step is 16 consecutive columns of one row.
//   * the 5 x 5 first layer (Cin = 3): the 15 values (kw, ci) of a kernel row are 15 consecutive bf16 of the image row.  The halo is
//     expanded in LDS to [halo row][column][16] (the sixteenth zero), 32 bytes a position; a 32-column MFMA block is two kernel rows
//     (the lanes' upper half reads one halo row further down), three blocks cover the five rows, the fourth wave adds the bias gradient.
//   * the bias gradient is one more MFMA per K-step against a fragment of ones: the same float32 accumulation, no extra pass.
//   * the sum is split over the tiles: split s owns tiles [s T, (s + 1) T) and writes one float32 partial [Cout][k][k][Cin] tile and one
//     [Cout] row; a second launch (ssd7_reduce_kernel, ssdhip_ssd7.h) adds the splits in index order in float32 and writes dw and db
//     once -- float32, or rounded once to bf16 -- through the parameter's element strides.  No atomics, no last-workgroup finish.
//     The number of splits is host arithmetic (ssdhip_ssd7_conv_wgrad_plan): the partial tiles, written and read back, must not exceed
//     the operand bytes the launch reads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_bf16.h"
#include "ssdhip_ssd7.h"

namespace ssdhip {
namespace {

constexpr int W7_MAX_SPLITS = 256;                       // the part's CU count: a constant, so that the plan is host arithmetic
constexpr int W7_TAIL = 64;                              // LDS behind the last image: what the padded lanes of its last position reach

struct W7Params {
    const unsigned char* x;      // [B, H, W, Cin] bf16
    const unsigned char* dy;     // [B, H, W, Cout] bf16
    float* part;                 // [splits][Cout k k Cin + Cout]
    int B, H, W;
    int HT, WT, tiles, tiles_per_split;
};

struct W7Plan {
    int splits, tiles_per_split, tiles, last_tiles;
};

long long w7_slot_floats(int Cin, int Cout, int kernel) { return (long long)Cout * kernel * kernel * Cin + Cout; }

// The plan, and with it the tile fields of the kernel's arguments (p.B .. p.tiles, p.tiles_per_split).
bool w7_plan(int B, int H, int W, int Cin, int Cout, int kernel, W7Plan& pl, W7Params& p) {
    if (!ssd7_geometry(Cin, Cout, kernel) || !ssd7_tile_grid(B, H, W, p)) return false;
    const long long tiles = p.tiles, operand = (long long)B * H * W * (Cin + Cout) * 2, slot = w7_slot_floats(Cin, Cout, kernel) * 4;
    long long most = operand / (2 * slot);               // a partial tile is written once and read once
    most = most > W7_MAX_SPLITS ? W7_MAX_SPLITS : most;
    most = most > tiles ? tiles : most;
    most = most < 1 ? 1 : most;
    pl.tiles = p.tiles;
    pl.tiles_per_split = p.tiles_per_split = (int)((tiles + most - 1) / most);
    pl.splits = (pl.tiles + pl.tiles_per_split - 1) / pl.tiles_per_split;
    pl.last_tiles = pl.tiles - (pl.splits - 1) * pl.tiles_per_split;
    return true;
}

// the dy tile, [8 x 32 positions][COUT + 8] in LDS: 16-byte chunks dealt to the threads, zeros outside the image
template <int COUT>
struct W7Dy {
    static constexpr int DS = COUT * 2 + 16, CH = COUT / 8, NLD = S7_TH * S7_TW * CH / S7_THREADS, BYTES = S7_TH * S7_TW * DS;
    static_assert(S7_TH * S7_TW * CH % S7_THREADS == 0, "whole chunks per thread");

    static __device__ __forceinline__ void fetch(const W7Params& p, int tile, int tid, u32x4 (&r)[NLD]) {
        int b, h0, w0;
        ssd7_tile_origin(p, tile, b, h0, w0);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int n = tid + S7_THREADS * i, px = n / CH, c = n - px * CH, h = h0 + (px >> 5), w = w0 + (px & 31);
            r[i] = u32x4{0u, 0u, 0u, 0u};
            if (h < p.H && w < p.W) r[i] = *reinterpret_cast<const u32x4*>(p.dy + (((size_t)b * p.H + h) * p.W + w) * (COUT * 2) + c * 16);
        }
    }
    static __device__ __forceinline__ void stash(unsigned char* dl, int tid, const u32x4 (&r)[NLD]) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int n = tid + S7_THREADS * i, px = n / CH, c = n - px * CH;
            *reinterpret_cast<u32x4*>(dl + px * DS + c * 16) = r[i];
        }
    }
};

// ---- 3 x 3 ------------------------------------------------------------------------------------------------------------------------
// LDS: halo [10 x 34 positions][Cin + 8] (S7Halo3) | dy tile [8 x 32][Cout + 8] | tail.
template <int CIN, int COUT>
struct W73 {
    using Dy = W7Dy<COUT>;
    using Halo = S7Halo3<CIN>;
    static constexpr int MT = (COUT + 31) / 32, NT = (CIN + 31) / 32, UNITS = MT * NT, TG = 4 / UNITS, NTAP = TG == 1 ? 9 : 5;
    static constexpr int HBYTES = Halo::BYTES, LDS = HBYTES + Dy::BYTES + W7_TAIL;
    static_assert(UNITS == 2 || UNITS == 4, "four waves share the 32 x 32 blocks");
    static_assert(LDS <= 160 * 1024 && HBYTES % 16 == 0, "LDS budget and alignment");
};

template <int CIN, int COUT>
__global__ __launch_bounds__(S7_THREADS) void wgrad7_k3_kernel(const W7Params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using G = W73<CIN, COUT>;
    using Dy = typename G::Dy;
    using Halo = typename G::Halo;
    constexpr int NT = G::NT, UNITS = G::UNITS, NTAP = G::NTAP, DS = Dy::DS;
    constexpr int PS = Halo::PS, CH = Halo::CH, HC = Halo::HC, NCHUNK = Halo::NCHUNK, NLD = Halo::NLD;
    extern __shared__ __attribute__((aligned(16))) unsigned char w7_lds[];
    unsigned char* hl = w7_lds;
    unsigned char* dl = w7_lds + G::HBYTES;
    s7_lds_byte* const ldsp = (s7_lds_byte*)w7_lds;

    const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, khalf = lane >> 5, i16 = lane & 15, g16 = (lane >> 4) & 1;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int unit = wave % UNITS, tg = wave / UNITS, mt = unit / NT, nt = unit - mt * NT;
    const int t0 = tg * 5, ntaps = G::TG == 1 ? 9 : (tg ? 4 : 5);
    const int split = (int)blockIdx.x;
    int tile = split * p.tiles_per_split;
    int end = tile + p.tiles_per_split;
    end = end > p.tiles ? p.tiles : end;

    // the halo's chunks (S7Halo3), as in convbn3_kernel
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

    // the lane's row inside a K-step and its 8 bytes of the 32-channel block (ssd7_fragment)
    const u32 lrow = (u32)(khalf * 4 + (i16 >> 2)), lcol = (u32)(g16 * 32 + (i16 & 3) * 8);
    const u32 a_lane = (u32)G::HBYTES + lrow * DS + (u32)(mt * 64) + lcol;
    const u32 b_lane = lrow * PS + (u32)(nt * 64) + lcol;
    u32 toff[NTAP];                                      // tap displacements in the halo (a wave's surplus slot repeats tap 8: not stored)
#pragma unroll
    for (int j = 0; j < NTAP; ++j) {
        const int t = t0 + j < 9 ? t0 + j : 8;
        toff[j] = (u32)(((t / 3) * HC + (t % 3)) * PS);
    }
    const bool sums = nt == 0 && tg == 0;                // this wave also adds the bias gradient of its 32 output channels
    const u32 one2 = 0x3f803f80u;
    const bf16x8 ones = __builtin_bit_cast(bf16x8, (u32x4{one2, one2, one2, one2}));

    f32x16 acc[NTAP], accb;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        accb[v] = 0.f;
#pragma unroll
        for (int j = 0; j < NTAP; ++j) acc[j][v] = 0.f;
    }

    u32x4 rx[NLD], rd[Dy::NLD];
    fetch(tile, rx);
    Dy::fetch(p, tile, tid, rd);
    for (; tile < end; ++tile) {
        stash(rx);
        Dy::stash(dl, tid, rd);
        __syncthreads();                                 // this tile's halo and dy are in LDS
        if (tile + 1 < end) {                            // in flight during the MFMAs
            fetch(tile + 1, rx);
            Dy::fetch(p, tile + 1, tid, rd);
        }
#pragma unroll 1
        for (int r = 0; r < S7_TH; ++r)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const bf16x8 a = __builtin_bit_cast(bf16x8, ssd7_fragment(ldsp, a_lane + (u32)((r * S7_TW + hf * 16) * DS), 8 * DS));
                const u32 b0 = b_lane + (u32)((r * HC + hf * 16) * PS);
#pragma unroll
                for (int j = 0; j < NTAP; ++j) {
                    const bf16x8 b = __builtin_bit_cast(bf16x8, ssd7_fragment(ldsp, b0 + toff[j], 8 * PS));
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
                }
                if (sums) accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, accb, 0, 0, 0);
            }
        __syncthreads();                                 // every wave is done with the tile before the next one overwrites it
    }

    // partial tile: the lane's column is input channel nt 32 + r31, register v output channel ssd7_acc_row
    float* out = p.part + (size_t)split * (COUT * 9 * CIN + COUT);
    const int ci = nt * 32 + r31;
#pragma unroll
    for (int j = 0; j < NTAP; ++j)
        if (j < ntaps && ci < CIN) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int co = ssd7_acc_row(mt, v, khalf);
                if (co < COUT) out[((size_t)co * 9 + t0 + j) * CIN + ci] = acc[j][v];
            }
        }
    if (sums && r31 == 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int co = ssd7_acc_row(mt, v, khalf);
            if (co < COUT) out[COUT * 9 * CIN + co] = accb[v];
        }
    }
#endif
}

// ---- 5 x 5, Cin = 3, Cout = 32 ------------------------------------------------------------------------------------------------
// LDS: halo [12 rows][224 bytes] (108 bf16 of 36 pixels: S7Halo5) | expanded [12 rows][32 columns][16 bf16]
// (element j = 3 kw + ci of column c is halo element 3 c + j; j = 15 zero) | dy tile [8 x 32][32 + 8] | tail.
constexpr int W75_HR = S7Halo5::HR, W75_HBYTES = S7Halo5::BYTES, W75_EBYTES = W75_HR * S7_TW * 32;
[[maybe_unused]] constexpr int W75_LDS = W75_HBYTES + W75_EBYTES + W7Dy<32>::BYTES + W7_TAIL;

__global__ __launch_bounds__(S7_THREADS) void wgrad7_k5_kernel(const W7Params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using Dy = W7Dy<32>;
    using Halo = S7Halo5;
    constexpr int DS = Dy::DS;
    __shared__ __attribute__((aligned(16))) unsigned char w7_lds[W75_LDS];
    unsigned char* hl = w7_lds;
    unsigned char* el = w7_lds + W75_HBYTES;
    unsigned char* dl = el + W75_EBYTES;
    s7_lds_byte* const ldsp = (s7_lds_byte*)w7_lds;

    const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, khalf = lane >> 5, i16 = lane & 15, g16 = (lane >> 4) & 1;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = (int)blockIdx.x;
    int tile = split * p.tiles_per_split;
    int end = tile + p.tiles_per_split;
    end = end > p.tiles ? p.tiles : end;
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
    // halo -> expanded image: position (hr, c) takes the 15 halo elements from 3 c on and a zero
    auto expand = [&]() {
        for (int n = tid; n < W75_HR * S7_TW; n += S7_THREADS) {
            const int hr = n >> 5, c = n & 31;
            const unsigned short* src = reinterpret_cast<const unsigned short*>(hl + hr * Halo::RS) + 3 * c;
            u32 d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = (u32)src[2 * j] | (j < 7 ? (u32)src[2 * j + 1] << 16 : 0u);
            u32x4* dst = reinterpret_cast<u32x4*>(el + n * 32);
            dst[0] = u32x4{d[0], d[1], d[2], d[3]};
            dst[1] = u32x4{d[4], d[5], d[6], d[7]};
        }
    };

    // waves 0 .. 2: kernel rows 2 wave + g16 (the last block's upper half repeats row 4 and is not stored); wave 3: the bias gradient
    const int kh = 2 * wave + g16 < 4 ? 2 * wave + g16 : 4;
    const u32 lrow = (u32)(khalf * 4 + (i16 >> 2));
    const u32 a_lane = (u32)(W75_HBYTES + W75_EBYTES) + lrow * DS + (u32)(g16 * 32 + (i16 & 3) * 8);
    const u32 b_lane = (u32)W75_HBYTES + (u32)((kh * S7_TW + lrow) * 32 + (i16 & 3) * 8);
    const u32 one2 = 0x3f803f80u;
    const bf16x8 ones = __builtin_bit_cast(bf16x8, (u32x4{one2, one2, one2, one2}));

    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;

    unsigned short rx[Halo::NLD];
    u32x4 rd[Dy::NLD];
    fetch(tile, rx);
    Dy::fetch(p, tile, tid, rd);
    for (; tile < end; ++tile) {
        stash(rx);
        Dy::stash(dl, tid, rd);
        __syncthreads();
        if (tile + 1 < end) {
            fetch(tile + 1, rx);
            Dy::fetch(p, tile + 1, tid, rd);
        }
        expand();
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < S7_TH; ++r)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const bf16x8 a = __builtin_bit_cast(bf16x8, ssd7_fragment(ldsp, a_lane + (u32)((r * S7_TW + hf * 16) * DS), 8 * DS));
                bf16x8 b = ones;
                if (wave < 3) b = __builtin_bit_cast(bf16x8, ssd7_fragment(ldsp, b_lane + (u32)((r * S7_TW + hf * 16) * 32), 8 * 32));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            }
        __syncthreads();
    }

    float* out = p.part + (size_t)split * (32 * 75 + 32);
    if (wave < 3) {
        if (2 * wave + g16 < 5 && i16 < 15) {
#pragma unroll
            for (int v = 0; v < 16; ++v) out[ssd7_acc_row(0, v, khalf) * 75 + kh * 15 + i16] = acc[v];
        }
    } else if (r31 == 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) out[32 * 75 + ssd7_acc_row(0, v, khalf)] = acc[v];
    }
#endif
}

}  // namespace
}  // namespace ssdhip

using namespace ssdhip;

extern "C" int ssdhip_ssd7_conv_wgrad_plan(int B, int H, int W, int Cin, int Cout, int kernel, int* plan) {
    W7Plan pl;
    W7Params p;
    if (!plan || !w7_plan(B, H, W, Cin, Cout, kernel, pl, p)) return SSDHIP_E_BADARG;
    plan[0] = pl.splits; plan[1] = pl.tiles_per_split; plan[2] = pl.tiles; plan[3] = pl.last_tiles;
    return SSDHIP_OK;
}

extern "C" size_t ssdhip_ssd7_conv_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int kernel) {
    W7Plan pl;
    W7Params p;
    if (!w7_plan(B, H, W, Cin, Cout, kernel, pl, p)) return 0;
    return (size_t)pl.splits * (size_t)w7_slot_floats(Cin, Cout, kernel) * 4;
}

extern "C" int ssdhip_ssd7_conv_wgrad_nhwc_bf16(const void* x, const void* dy, void* dw, void* db, int B, int H, int W, int Cin, int Cout,
                                                int kernel, int out_bf16, const long long* dw_strides, void* workspace,
                                                size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    W7Plan pl;
    W7Params p;
    if (!x || !dy || !dw || !workspace || !w7_plan(B, H, W, Cin, Cout, kernel, pl, p)) return SSDHIP_E_BADARG;
    if (workspace_bytes < (size_t)pl.splits * (size_t)w7_slot_floats(Cin, Cout, kernel) * 4) return SSDHIP_E_BADARG;
    const uintptr_t omask = out_bf16 ? 1 : 3;
    if (((uintptr_t)x & (kernel == 3 ? 15 : 1)) || (((uintptr_t)dy | (uintptr_t)workspace) & 15) || (((uintptr_t)dw | (uintptr_t)db) & omask))
        return SSDHIP_E_BADARG;
    S7Reduce q = {};                                     // one destination: every row of the tile is dw's, db may be NULL
    if (!ssd7_strides(dw_strides, Cout, Cin, kernel, q.s[0])) return SSDHIP_E_BADARG;
    p.x = static_cast<const unsigned char*>(x); p.dy = static_cast<const unsigned char*>(dy); p.part = static_cast<float*>(workspace);
    int rc = SSDHIP_E_BADARG;
    if (kernel == 5)
        rc = ssd7_launch<wgrad7_k5_kernel>(dim3(pl.splits), 0, 0, stream, p);
    else
        ssd7_for_pair3(Cin, Cout, [&](auto ci, auto co) {
            constexpr int CIN = decltype(ci)::value, COUT = decltype(co)::value, LDS = W73<CIN, COUT>::LDS;
            rc = ssd7_launch<wgrad7_k3_kernel<CIN, COUT>>(dim3(pl.splits), LDS, LDS, stream, p);
        });
    if (rc != SSDHIP_OK) return rc;
    q.part = p.part; q.dw[0] = dw; q.db[0] = db; q.n[0] = q.rows = Cout; q.slots = pl.splits; q.cin = Cin; q.kernel = kernel;
    q.out_bf16 = out_bf16 ? 1 : 0;
    return ssd7_reduce(q, stream);
}
