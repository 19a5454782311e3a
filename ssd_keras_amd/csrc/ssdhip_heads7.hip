// ssdhip_heads7.hip -- the predictor heads of SSD7's training step (reference models/keras_ssd7.py:323-331: `classes4..7` and `boxes4..7`,
// Conv2D(3 x 3, 'same') on the 64 / 48 / 48 / 32-channel maps conv4..conv7), gfx950.  The two heads of a source map run as ONE
// convolution whose filters are [conf | loc | zero rows] up to Cp = 48 output channels: forward and data gradient are
// ssdhip_conv_same_bias_nhwc_bf16 (csrc/ssdhip_convbn.hip) on the geometries (Cin, 48) and (48, Cin) it already has.  This file adds
//   * ssdhip_ssd7_pack_heads: ONE launch that writes, for up to eight maps, the forward filter image of the concatenated weight, the
//     image of its flip / transpose (the data gradient's filters) and the packed bf16 bias, from the four bf16 parameters through their
//     element strides.  Every byte of every buffer is written; the table of tensors travels in the kernel arguments.
//   * ssdhip_ssd7_head_wgrad_nhwc_bf16: the weight and bias gradients of both heads from x [B, H, W, Cin] and the packed dL/dy
//     [B, H, W, 48], bf16 NHWC, float32 accumulation on v_mfma_f32_32x32x16_bf16.
//
// The weight gradient on small maps.  ssdhip_ssd7_conv_wgrad_nhwc_bf16 (csrc/ssdhip_wgrad7.hip) walks 8 x 32 position tiles per image;
// on a 9 x 9 or 4 x 4 map 84 % / 94 % of what it multiplies is tile padding.  Here the batch is ONE list of positions on a zero-padded
// grid: image b is (H + 2) x (W + 2) with a border of zero pixels, image after image, P = B (H + 2)(W + 2) positions, and dL/dy lies on
// the same grid with zeros on the border.  Then
//     dw[co][kh][kw][ci] = sum_q dy_pad[q][co] x_pad[q + (kh - 1)(W + 2) + (kw - 1)][ci]
// -- a tap is a CONSTANT displacement in the list.  Where q is a border position dy_pad is zero; where q is an interior position its
// nine neighbours lie inside its own padded image; so row wrap-around and image borders add nothing and nothing is masked.  The
// useful share of the contraction is H W / ((H + 2)(W + 2)): 90 / 81 / 67 / 44 % on 37 / 18 / 9 / 4-pixel maps.
//   * a workgroup of four waves walks chunks of 256 list positions.  Per chunk the loader writes the dy rows [256][48 + 8] and the x
//     rows [256 + 2 (W + 3)][Cin + 8] into LDS -- zeros on the border and outside the list, written by the loader itself -- and both
//     operands are read with ds_read_b64_tr_b16 through ssd7_fragment (ssdhip_ssd7.h: a lane gets four consecutive positions of its
//     channel; 48 channels run as two 32-channel blocks whose upper 16 lanes read what lies behind the row, inside the allocation, and
//     whose results are never stored).  A tap displaces the x row address by a multiple of the row pitch: always 8-byte aligned.
//   * the work is split over position chunks (grid x: split s owns chunks [s T, (s + 1) T)) AND over the three kernel rows (grid y),
//     so a 4 x 4 map at batch 32 still occupies 3 x 5 workgroups; a kernel row's workgroup holds 3 taps x (Cout, Cin) 32 x 32 blocks in
//     accumulators, one block per wave.  Cin = 32 has only two blocks: its second pair of waves takes the odd 16-position steps and
//     writes a partial tile of its own.  The kernel row kh = 1 also adds the bias gradient (one more MFMA per step against ones).
//   * every (split, step parity) writes one float32 partial [48][3][3][Cin] + [48], each element exactly once (the three kernel rows
//     write disjoint thirds); a second launch (ssd7_reduce_kernel) adds the partials in index order in float32 and writes dw_conf, db_conf, dw_loc and
//     db_loc once -- float32, or rounded once to bf16 -- through the parameters' element strides, dropping the padding rows.
//     Bit-reproducible; no atomics, no last-workgroup finish, no memset.  The plan is host arithmetic on the shape only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_bf16.h"
#include "ssdhip_ssd7.h"

namespace ssdhip {
namespace {

constexpr int H7_CP = 48;                               // packed output channels
constexpr int H7_CHUNK = 256;                            // list positions per chunk: 16 MFMA steps of 16
constexpr int H7_MIN_SPLITS = 8, H7_MAX_SPLITS = 64;     // x 3 kernel rows = 24 .. 192 workgroups
constexpr int H7_MAX_W = 256;                            // x rows in LDS: 256 + 2 (W + 3), at most 774 x 144 bytes
constexpr int H7_DS = H7_CP * 2 + 16;                    // dy row pitch
constexpr int H7_TAIL = 64;                              // LDS behind the last dy row: what the padded lanes of that row reach
constexpr int H7_PACK_MAX = 8;

struct H7Plan {
    int splits, chunks_per_split, chunks, last_chunks, positions, ksplit;
};

bool h7_cin(int Cin) { return Cin == 64 || Cin == 48 || Cin == 32; }
long long h7_slot_floats(int Cin) { return (long long)H7_CP * 9 * Cin + H7_CP; }
size_t h7_lds_bytes(int W, int Cin) { return (size_t)(H7_CHUNK + 2 * (W + 3)) * (Cin * 2 + 16) + (size_t)H7_CHUNK * H7_DS + H7_TAIL; }

// The split: as many as keep the partial tiles a launch writes within the operand bytes it reads, but at least 8 (the tiles of the
// small maps stay in the cache, and one workgroup per kernel row would walk every chunk alone), at most 64, at most one per chunk.
bool h7_plan(int B, int H, int W, int Cin, int Cp, H7Plan& pl) {
    if (B <= 0 || H <= 0 || W <= 0 || W > H7_MAX_W || Cp != H7_CP || !h7_cin(Cin)) return false;
    const long long positions = (long long)B * (H + 2) * (W + 2);
    if (positions > S7_MAX_INDEX) return false;
    const long long chunks = (positions + H7_CHUNK - 1) / H7_CHUNK;
    const int ksplit = Cin == 32 ? 2 : 1;
    const long long operand = (long long)B * H * W * (Cin + H7_CP) * 2, slot = h7_slot_floats(Cin) * 4 * ksplit;
    long long most = operand / slot;
    most = most < H7_MIN_SPLITS ? H7_MIN_SPLITS : most;
    most = most > H7_MAX_SPLITS ? H7_MAX_SPLITS : most;
    most = most > chunks ? chunks : most;
    pl.positions = (int)positions;
    pl.chunks = (int)chunks;
    pl.chunks_per_split = (int)((chunks + most - 1) / most);
    pl.splits = (pl.chunks + pl.chunks_per_split - 1) / pl.chunks_per_split;
    pl.last_chunks = pl.chunks - (pl.splits - 1) * pl.chunks_per_split;
    pl.ksplit = ksplit;
    return true;
}

struct H7Params {
    const unsigned char* x;      // [B, H, W, Cin] bf16
    const unsigned char* dy;     // [B, H, W, 48] bf16
    float* part;                 // [splits ksplit][48 x 9 x Cin + 48]
    int H, W;
    int positions, chunks, chunks_per_split;
};

// rows [first, first + rows) of the padded list of a [B, H, W, C] map into LDS at `pitch` bytes a row: 16-byte pieces dealt to the
// threads; a border pixel and a position outside the list are zeros
template <int C>
__device__ __forceinline__ void h7_load_rows(const unsigned char* src, unsigned char* lds, int pitch, int first, int rows, int H, int W,
                                             int positions, int tid) {
    constexpr int CH = C / 8;
    const int Wp = W + 2, plane = (H + 2) * Wp;
    for (int n = tid; n < rows * CH; n += S7_THREADS) {
        const int j = n / CH, c = n - j * CH, q = first + j;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (q >= 0 && q < positions) {
            const int b = q / plane, r = q - b * plane, rr = r / Wp, cc = r - rr * Wp;
            if (rr >= 1 && rr <= H && cc >= 1 && cc <= W)
                v = *reinterpret_cast<const u32x4*>(src + (((size_t)b * H + (rr - 1)) * W + (cc - 1)) * (C * 2) + c * 16);
        }
        *reinterpret_cast<u32x4*>(lds + (size_t)j * pitch + c * 16) = v;
    }
}

// LDS: x rows [256 + 2 (W + 3)][Cin + 8] | dy rows [256][48 + 8] | tail.  x row j is list position chunk 256 - (W + 3) + j.
template <int CIN>
__global__ __launch_bounds__(S7_THREADS) void head_wgrad_kernel(const H7Params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NT = (CIN + 31) / 32, UNITS = 2 * NT, KSPLIT = 4 / UNITS, PS = CIN * 2 + 16, DS = H7_DS;
    static_assert(UNITS == 2 || UNITS == 4, "four waves share the 32 x 32 blocks");
    extern __shared__ __attribute__((aligned(16))) unsigned char h7_lds[];
    const int Wp = p.W + 2, halo = Wp + 1, xrows = H7_CHUNK + 2 * halo;
    unsigned char* xl = h7_lds;
    unsigned char* dl = h7_lds + (size_t)xrows * PS;
    s7_lds_byte* const ldsp = (s7_lds_byte*)h7_lds;

    const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, khalf = lane >> 5, i16 = lane & 15, g16 = (lane >> 4) & 1;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int unit = wave % UNITS, ks = wave / UNITS, mt = unit / NT, nt = unit - mt * NT;
    const int kh = (int)blockIdx.y, split = (int)blockIdx.x;
    int chunk = split * p.chunks_per_split;
    int end = chunk + p.chunks_per_split;
    end = end > p.chunks ? p.chunks : end;

    // the lane's row inside a step and its 8 bytes of the 32-channel block (ssd7_fragment)
    const u32 lrow = (u32)(khalf * 4 + (i16 >> 2)), lcol = (u32)(g16 * 32 + (i16 & 3) * 8);
    const u32 a_lane = (u32)(xrows * PS) + lrow * DS + (u32)(mt * 64) + lcol;
    const u32 b_lane = lrow * PS + (u32)(nt * 64) + lcol;
    u32 toff[3];                                         // the kernel row's three taps: displacements in the list
#pragma unroll
    for (int j = 0; j < 3; ++j) toff[j] = (u32)((halo + (kh - 1) * Wp + (j - 1)) * PS);
    const bool sums = kh == 1 && nt == 0;                // this wave also adds the bias gradient of its 32 output channels
    const u32 one2 = 0x3f803f80u;
    const bf16x8 ones = __builtin_bit_cast(bf16x8, (u32x4{one2, one2, one2, one2}));

    f32x16 acc[3], accb;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        accb[v] = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j][v] = 0.f;
    }

    for (; chunk < end; ++chunk) {
        const int q0 = chunk * H7_CHUNK;
        h7_load_rows<CIN>(p.x, xl, PS, q0 - halo, xrows, p.H, p.W, p.positions, tid);
        h7_load_rows<H7_CP>(p.dy, dl, DS, q0, H7_CHUNK, p.H, p.W, p.positions, tid);
        __syncthreads();                                 // this chunk's rows are in LDS
#pragma unroll 2
        for (int s = ks; s < H7_CHUNK / 16; s += KSPLIT) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, ssd7_fragment(ldsp, a_lane + (u32)(s * 16 * DS), 8 * DS));
            const u32 b0 = b_lane + (u32)(s * 16 * PS);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const bf16x8 b = __builtin_bit_cast(bf16x8, ssd7_fragment(ldsp, b0 + toff[j], 8 * PS));
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
            }
            if (sums) accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, accb, 0, 0, 0);
        }
        __syncthreads();                                 // every wave is done with the chunk before the next one overwrites it
    }

    // partial tile of this (split, step parity): the lane's column is input channel nt 32 + r31, register v output channel ssd7_acc_row
    float* out = p.part + (size_t)(split * KSPLIT + ks) * (H7_CP * 9 * CIN + H7_CP);
    const int ci = nt * 32 + r31;
    if (ci < CIN) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int co = ssd7_acc_row(mt, v, khalf);
                if (co < H7_CP) out[((size_t)co * 9 + 3 * kh + j) * CIN + ci] = acc[j][v];
            }
    }
    if (sums && r31 == 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int co = ssd7_acc_row(mt, v, khalf);
            if (co < H7_CP) out[H7_CP * 9 * CIN + co] = accb[v];
        }
    }
#endif
}

// the kernel of a Cin, its dynamic LDS allowed up to what the widest map needs
template <int CIN>
int h7_launch(const H7Params& p, const H7Plan& pl, size_t lds, hipStream_t stream) {
    return ssd7_launch<head_wgrad_kernel<CIN>>(dim3(pl.splits, 3), (int)h7_lds_bytes(H7_MAX_W, CIN), lds, stream, p);
}

// ---- the packed images and bias of the heads, refreshed on the device --------------------------------------------------------------
struct H7PackMap {
    const bf16_t* w[2];          // conf, loc filters (n, Cin, 3, 3) through their element strides
    const bf16_t* b[2];          // conf, loc bias, dense
    bf16_t* fwd;                 // [3][3][64][Cin + 8]: the image of ssdhip_conv_bn_elu_pack_bytes(Cin, 48, 3)
    bf16_t* flip;                // [3][3][Cin rounded up to 32][48 + 8]: ... (48, Cin, 3), of the flipped / transposed filters
    bf16_t* bias;                // [48]
    long long s[2][4];
    int cin, n[2];
};
struct H7PackTable {
    H7PackMap map[H7_PACK_MAX];
};

// packed filter (row r of 48, input channel c, tap kh, kw): conf rows, then loc rows, then zeros
__device__ __forceinline__ bf16_t h7_packed_filter(const H7PackMap& M, int r, int c, int kh, int kw) {
    if (r >= M.n[0] + M.n[1]) return (bf16_t)0;
    const int head = r >= M.n[0];
    if (head) r -= M.n[0];
    return M.w[head][r * M.s[head][0] + c * M.s[head][1] + kh * M.s[head][2] + kw * M.s[head][3]];
}

__global__ __launch_bounds__(S7_THREADS) void head_pack_kernel(const H7PackTable t) {
    const H7PackMap& M = t.map[blockIdx.y / 3];
    const int what = (int)(blockIdx.y % 3);
    const int step = (int)(gridDim.x * blockDim.x), first = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (what == 2) {
        for (int i = first; i < H7_CP; i += step)
            M.bias[i] = i < M.n[0] ? M.b[0][i] : (i < M.n[0] + M.n[1] ? M.b[1][i - M.n[0]] : (bf16_t)0);
        return;
    }
    const bool flip = what == 1;                         // forward: (48, Cin); flipped: (Cin, 48), rows / columns swapped and taps flipped
    ssd7_write_image3(flip ? M.flip : M.fwd, flip ? M.cin : H7_CP, flip ? H7_CP : M.cin, first, step, [&](int r, int c, int kh, int kw) {
        return flip ? h7_packed_filter(M, c, r, 2 - kh, 2 - kw) : h7_packed_filter(M, r, c, kh, kw);
    });
}

}  // namespace
}  // namespace ssdhip

using namespace ssdhip;

extern "C" int ssdhip_ssd7_pack_heads(int n_maps, const void* const* conf_w, const void* const* loc_w, const void* const* conf_b,
                                      const void* const* loc_b, void* const* fwd, void* const* flipped, void* const* bias, const int* Cin,
                                      const int* n_conf, const int* n_loc, const long long* strides, void* stream_) {
    if (n_maps <= 0 || n_maps > H7_PACK_MAX || !conf_w || !loc_w || !conf_b || !loc_b || !fwd || !flipped || !bias || !Cin || !n_conf ||
        !n_loc || !strides)
        return SSDHIP_E_BADARG;
    H7PackTable t = {};
    for (int i = 0; i < n_maps; ++i) {
        H7PackMap& M = t.map[i];
        if (!conf_w[i] || !loc_w[i] || !conf_b[i] || !loc_b[i] || !fwd[i] || !flipped[i] || !bias[i]) return SSDHIP_E_BADARG;
        if (!h7_cin(Cin[i]) || n_conf[i] <= 0 || n_loc[i] <= 0 || n_conf[i] + n_loc[i] > H7_CP) return SSDHIP_E_BADARG;
        if (((uintptr_t)conf_w[i] | (uintptr_t)loc_w[i] | (uintptr_t)conf_b[i] | (uintptr_t)loc_b[i] | (uintptr_t)fwd[i] |
             (uintptr_t)flipped[i] | (uintptr_t)bias[i]) & 1)
            return SSDHIP_E_BADARG;
        for (int h = 0; h < 2; ++h)
            if (!ssd7_strides(strides + 8 * i + 4 * h, h ? n_loc[i] : n_conf[i], Cin[i], 3, M.s[h])) return SSDHIP_E_BADARG;
        M.w[0] = static_cast<const bf16_t*>(conf_w[i]); M.w[1] = static_cast<const bf16_t*>(loc_w[i]);
        M.b[0] = static_cast<const bf16_t*>(conf_b[i]); M.b[1] = static_cast<const bf16_t*>(loc_b[i]);
        M.fwd = static_cast<bf16_t*>(fwd[i]); M.flip = static_cast<bf16_t*>(flipped[i]); M.bias = static_cast<bf16_t*>(bias[i]);
        M.cin = Cin[i]; M.n[0] = n_conf[i]; M.n[1] = n_loc[i];
    }
    const int bx = (ssd7_image3_elems(64, 64) + S7_THREADS * 4 - 1) / (S7_THREADS * 4);      // about four elements a thread in the largest image
    return ssd7_launch<head_pack_kernel>(dim3(bx, 3 * n_maps), 0, 0, static_cast<hipStream_t>(stream_), t);
}

extern "C" int ssdhip_ssd7_head_wgrad_plan(int B, int H, int W, int Cin, int Cp, int* plan) {
    H7Plan pl;
    if (!plan || !h7_plan(B, H, W, Cin, Cp, pl)) return SSDHIP_E_BADARG;
    plan[0] = pl.splits; plan[1] = pl.chunks_per_split; plan[2] = pl.chunks; plan[3] = pl.last_chunks;
    plan[4] = H7_CHUNK; plan[5] = 3; plan[6] = pl.ksplit; plan[7] = pl.positions;
    return SSDHIP_OK;
}

extern "C" size_t ssdhip_ssd7_head_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cp) {
    H7Plan pl;
    if (!h7_plan(B, H, W, Cin, Cp, pl)) return 0;
    return (size_t)pl.splits * pl.ksplit * (size_t)h7_slot_floats(Cin) * 4;
}

extern "C" int ssdhip_ssd7_head_wgrad_nhwc_bf16(const void* x, const void* dy, void* dw_conf, void* db_conf, void* dw_loc, void* db_loc, int B,
                                                int H, int W, int Cin, int Cp, int n_conf, int n_loc, int out_bf16,
                                                const long long* dw_conf_strides, const long long* dw_loc_strides, void* workspace,
                                                size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    H7Plan pl;
    if (!x || !dy || !dw_conf || !db_conf || !dw_loc || !db_loc || !workspace || !h7_plan(B, H, W, Cin, Cp, pl)) return SSDHIP_E_BADARG;
    if (n_conf <= 0 || n_loc <= 0 || n_conf + n_loc > H7_CP) return SSDHIP_E_BADARG;
    if (workspace_bytes < (size_t)pl.splits * pl.ksplit * (size_t)h7_slot_floats(Cin) * 4) return SSDHIP_E_BADARG;
    const uintptr_t omask = out_bf16 ? 1 : 3;
    if ((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)workspace) & 15) ||
        (((uintptr_t)dw_conf | (uintptr_t)db_conf | (uintptr_t)dw_loc | (uintptr_t)db_loc) & omask))
        return SSDHIP_E_BADARG;
    S7Reduce q;                                          // two destinations: the conf head's rows, then the loc head's
    if (!ssd7_strides(dw_conf_strides, n_conf, Cin, 3, q.s[0]) || !ssd7_strides(dw_loc_strides, n_loc, Cin, 3, q.s[1])) return SSDHIP_E_BADARG;
    H7Params p;
    p.x = static_cast<const unsigned char*>(x); p.dy = static_cast<const unsigned char*>(dy); p.part = static_cast<float*>(workspace);
    p.H = H; p.W = W; p.positions = pl.positions; p.chunks = pl.chunks; p.chunks_per_split = pl.chunks_per_split;
    const size_t lds = h7_lds_bytes(W, Cin);
    const int rc = Cin == 64 ? h7_launch<64>(p, pl, lds, stream) : Cin == 48 ? h7_launch<48>(p, pl, lds, stream) : h7_launch<32>(p, pl, lds, stream);
    if (rc != SSDHIP_OK) return rc;
    q.part = p.part; q.dw[0] = dw_conf; q.dw[1] = dw_loc; q.db[0] = db_conf; q.db[1] = db_loc;
    q.slots = pl.splits * pl.ksplit; q.cin = Cin; q.kernel = 3; q.rows = H7_CP; q.n[0] = n_conf; q.n[1] = n_loc; q.out_bf16 = out_bf16 ? 1 : 0;
    return ssd7_reduce(q, stream);
}
