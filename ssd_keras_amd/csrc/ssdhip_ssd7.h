// ssdhip_ssd7.h -- what SSD7's three MFMA kernel files share: ssdhip_convbn.hip (forward and data gradient),
// ssdhip_wgrad7.hip (the trunk's weight gradient) and ssdhip_heads7.hip (head packing and head weight gradient).
//   host:   the seven geometries and the dispatcher from a runtime (Cin, Cout) to its compile-time pair, the 8 x 32 tile grid with its
//           limits, the element-stride check, the launch helper, the size of a 3 x 3 filter image;
//   device: the tile origin, the layouts of the 3 x 3 and 5 x 5 halos, the transpose-read fragment, the accumulator's row order, the
//           3 x 3 filter-image writer and the reduce kernel of both weight gradients.
// Everything has internal linkage, as the helpers of ssdhip_bf16.h: a file that includes this header compiles its own copy (the reduce
// kernel is in all three code objects, used by two).  Structs that travel as kernel arguments are not shared: the grid builder and the
// tile origin take any parameter struct with H, W, HT, WT ..., so every kernel keeps its own argument layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ssdhip.h"
#include "ssdhip_bf16.h"

namespace ssdhip {
namespace {

constexpr int S7_THREADS = 256;                          // four waves, in every kernel of the family
constexpr int S7_TH = 8, S7_TW = 32;                     // the position tile of the forward kernel and of the trunk's weight gradient
constexpr long long S7_MAX_INDEX = 0x3fffffffLL;         // positions, tiles and the reach of a stride set stay below 2^30

// ---- host: geometries ------------------------------------------------------------------------------------------------------------
// The 3 x 3 layers: f(integral_constant<int, Cin>, integral_constant<int, Cout>) for the pair that (Cin, Cout) is; false if it is none.
template <typename F>
bool ssd7_for_pair3(int Cin, int Cout, F&& f) {
    bool hit = false;
    auto on = [&](auto ci, auto co) {
        if (Cin != decltype(ci)::value || Cout != decltype(co)::value) return;
        hit = true;
        f(ci, co);
    };
    using std::integral_constant;
    on(integral_constant<int, 32>(), integral_constant<int, 48>());
    on(integral_constant<int, 48>(), integral_constant<int, 64>());
    on(integral_constant<int, 48>(), integral_constant<int, 48>());
    on(integral_constant<int, 48>(), integral_constant<int, 32>());
    on(integral_constant<int, 64>(), integral_constant<int, 64>());
    on(integral_constant<int, 64>(), integral_constant<int, 48>());
    return hit;
}

// exactly SSD7's seven convolutions: the six 3 x 3 pairs and the 5 x 5 first layer
bool ssd7_geometry(int Cin, int Cout, int kernel) {
    if (kernel == 5) return Cin == 3 && Cout == 32;
    return kernel == 3 && ssd7_for_pair3(Cin, Cout, [](auto, auto) {});
}

// elements of the filter image of a 3 x 3 layer, [tap][rows rounded up to 32][cols + 8] (forward: rows = Cout, cols = Cin)
__host__ __device__ inline int ssd7_image3_elems(int rows, int cols) { return 9 * ((rows + 31) / 32) * 32 * (cols + 8); }

// ---- host: the tile grid ---------------------------------------------------------------------------------------------------------
// Fills p.B, p.H, p.W, p.HT, p.WT and p.tiles = B HT WT; false for an empty map or one beyond the index limits.
template <class P>
bool ssd7_tile_grid(int B, int H, int W, P& p) {
    if (B <= 0 || H <= 0 || W <= 0) return false;
    p.B = B; p.H = H; p.W = W;
    p.HT = (H + S7_TH - 1) / S7_TH; p.WT = (W + S7_TW - 1) / S7_TW;
    const long long tiles = (long long)B * p.HT * p.WT;
    if (tiles > S7_MAX_INDEX || (long long)B * H * W > S7_MAX_INDEX) return false;
    p.tiles = (int)tiles;
    return true;
}

// ---- host: element strides -------------------------------------------------------------------------------------------------------
// s = the given element strides (rows, Cin, kh, kw) of a (rows, Cin, k, k) tensor, or dense [rows][k][k][Cin] for NULL.  false: a
// negative stride, or the farthest element they address (a sanity bound, not the tensor's size) beyond the index limit.
bool ssd7_strides(const long long* given, int rows, int Cin, int kernel, long long (&s)[4]) {
    s[0] = (long long)kernel * kernel * Cin; s[1] = 1; s[2] = (long long)kernel * Cin; s[3] = Cin;
    if (!given) return true;
    long long reach = 0;
    const int dims[4] = {rows, Cin, kernel, kernel};
    for (int d = 0; d < 4; ++d) {
        if (given[d] < 0) return false;
        s[d] = given[d];
        reach += given[d] * (dims[d] - 1);
    }
    return reach <= S7_MAX_INDEX;
}

// ---- host: launch ----------------------------------------------------------------------------------------------------------------
// S7_THREADS-wide workgroups of kernel FN.  lds_max > 0: the dynamic-LDS attribute is set first, once per kernel (the static belongs
// to this template's instantiation, and FN is its argument).
template <auto FN, class P>
int ssd7_launch(dim3 grid, int lds_max, size_t lds, hipStream_t stream, const P& p) {
    static const hipError_t attr =
        lds_max > 0 ? hipFuncSetAttribute(reinterpret_cast<const void*>(FN), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) : hipSuccess;
    if (attr != hipSuccess) return SSDHIP_E_LAUNCH;
    hipLaunchKernelGGL(FN, grid, dim3(S7_THREADS), lds, stream, p);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// ---- device: tiles and halos -----------------------------------------------------------------------------------------------------
template <class P>
__device__ __forceinline__ void ssd7_tile_origin(const P& p, int tile, int& b, int& h0, int& w0) {
    const int wt = tile % p.WT, q = tile / p.WT;
    b = q / p.HT;
    h0 = (q - b * p.HT) * S7_TH;
    w0 = wt * S7_TW;
}

// The 3 x 3 halo of a tile, [10 x 34 pixels][CIN + 8] in LDS: the 16 bytes of padding behind every pixel's CIN values keep the fragment
// reads of 32 consecutive rows off one bank set.  Its 16-byte chunks are dealt to the threads, NLD a thread.
// The layout is shared; the loader is not.  convbn3_kernel and wgrad7_k3_kernel each keep their own `fetch` / `stash` lambdas over these
// constants (and convbn5_kernel / wgrad7_k5_kernel over S7Halo5's), because the loaders sit inside the kernels' software pipelines:
// as member functions here (forced inline or not) and as closures handed out from here, the same loops compiled to other instruction
// streams with other VGPR counts (convbn3_kernel<64, 64>: 264 -> 248, wgrad7_k3_kernel<48, 64>: 412 -> 344) -- unmeasured code.
template <int CIN>
struct S7Halo3 {
    static constexpr int PS = CIN * 2 + 16, CH = CIN / 8, HR = S7_TH + 2, HC = S7_TW + 2, HPX = HR * HC, NCHUNK = HPX * CH;
    static constexpr int NLD = (NCHUNK + S7_THREADS - 1) / S7_THREADS, BYTES = HPX * PS;
};

// The 5 x 5 halo of the first layer (Cin = 3): 12 rows x 36 pixels x 3 channels = 108 bf16 a row, in 224-byte LDS rows, one bf16 a
// thread and step.
struct S7Halo5 {
    static constexpr int HR = S7_TH + 4, HC = S7_TW + 4, ROW = HC * 3, RS = 224, NEL = HR * ROW;
    static constexpr int NLD = (NEL + S7_THREADS - 1) / S7_THREADS, BYTES = HR * RS;
};

// ---- device: the weight gradients' operands ----------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) unsigned char s7_lds_byte;
typedef short s7_s16x4 __attribute__((ext_vector_type(4)));
// ds_read_b64_tr_b16: per 16 lanes a 4-row x 16-column block of 16-bit values; lane 4 q + p gives the address of row q, columns 4 p ..
// 4 p + 3, lane i receives column i of the four rows.  Two reads (rows + 0, + 8) make the fragment of a 16-position K-step: element j of
// lane half h is position 8 (j >> 2) + 4 h + (j & 3) -- in BOTH operands, which is all the MFMA asks of the K order.
__device__ __forceinline__ u32x4 ssd7_fragment(s7_lds_byte* lds, u32 off, u32 rows8) {
    const s7_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s7_s16x4*)(lds + off));
    const s7_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s7_s16x4*)(lds + off + rows8));
    const u32x2 l = __builtin_bit_cast(u32x2, lo), h = __builtin_bit_cast(u32x2, hi);
    return u32x4{l.x, l.y, h.x, h.y};
}
#endif

// The output channel that register v of the 32 x 32 accumulator block mt holds in lane half khalf; the lane's column is an input
// channel.  (The loops that store a partial tile with it stay in the two weight-gradient kernels: moved here, they too compiled to
// other code -- head_wgrad_kernel<64>: 890 -> 1064 instructions, 132 -> 136 VGPRs.)
__device__ __forceinline__ int ssd7_acc_row(int mt, int v, int khalf) { return mt * 32 + 8 * (v >> 2) + 4 * khalf + (v & 3); }

// dw / db = the partial tiles [slots][rows k k cin + rows] added in index order in float32 and written once: float32, or rounded once to
// bf16, dw through the parameter's element strides (Cout, Cin, kh, kw).  Up to two destinations: tile row co < n[0] is row co of the
// first, the next n[1] rows are the second's, the rest is padding and goes nowhere.  A NULL db is skipped.
struct S7Reduce {
    const float* part;
    void* dw[2];
    void* db[2];
    long long s[2][4];
    int n[2];
    int slots, cin, kernel, rows, out_bf16;
};

__global__ __launch_bounds__(S7_THREADS) void ssd7_reduce_kernel(const S7Reduce q) {
    const int kkc = q.kernel * q.kernel * q.cin, nw = q.rows * kkc, n = nw + q.rows;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    int co = i < nw ? i / kkc : i - nw;
    if (co >= q.n[0] + q.n[1]) return;
    float sum = q.part[i];
    for (int s = 1; s < q.slots; ++s) sum += q.part[(size_t)s * n + i];
    const int head = co >= q.n[0];
    if (head) co -= q.n[0];
    if (i < nw) {
        const int r = i % kkc, t = r / q.cin, ci = r - t * q.cin, kh = t / q.kernel, kw = t - kh * q.kernel;
        const long long at = co * q.s[head][0] + ci * q.s[head][1] + kh * q.s[head][2] + kw * q.s[head][3];
        if (q.out_bf16) static_cast<bf16_t*>(q.dw[head])[at] = bf16_bits<bf16_t>(sum);
        else static_cast<float*>(q.dw[head])[at] = sum;
    } else if (q.db[head]) {
        if (q.out_bf16) static_cast<bf16_t*>(q.db[head])[co] = bf16_bits<bf16_t>(sum);
        else static_cast<float*>(q.db[head])[co] = sum;
    }
}

int ssd7_reduce(const S7Reduce& q, hipStream_t stream) {
    const int n = q.rows * (q.kernel * q.kernel * q.cin + 1);
    return ssd7_launch<ssd7_reduce_kernel>(dim3((n + S7_THREADS - 1) / S7_THREADS), 0, 0, stream, q);
}

// ---- device: filter images ---------------------------------------------------------------------------------------------------------
// Every element of a 3 x 3 filter image [tap][rows rounded up to 32][cols + 8] (ssd7_image3_elems), i = first, first + step, ...:
// elem(r, c, kh, kw) inside, zero in the padding rows and columns.
template <class F>
__device__ __forceinline__ void ssd7_write_image3(bf16_t* out, int rows, int cols, int first, int step, F elem) {
    const int rp = (rows + 31) / 32 * 32, cp = cols + 8;
    for (int i = first; i < 9 * rp * cp; i += step) {
        const int c = i % cp, q = i / cp, r = q % rp, tap = q / rp, kh = tap / 3, kw = tap - 3 * kh;
        out[i] = r < rows && c < cols ? elem(r, c, kh, kw) : (bf16_t)0;
    }
}

}  // namespace
}  // namespace ssdhip
