// ssdhip_bntrain.hip -- SSD7's blocks in the TRAINING step, everything between a block's convolution and the next one's:
// BatchNormalization(axis=3) with BATCH statistics -> ELU(alpha=1) [-> MaxPooling2D(2, 2) 'valid'] (reference
// models/keras_ssd7.py:277-309) forward and backward.  gfx950, bf16 NHWC maps, float32 arithmetic, plain C++.
//
// Memory-bound streaming kernels: a lane owns 8 channels (16 bytes) of a pixel -- of a 2 x 2 window in the pooled forward forms --
// and C / 8 neighbouring lanes cover a pixel; C is 32, 48 or 64.  Every reduction has an order that depends on the shape alone:
// no atomics, no "last workgroup finishes", no memset; every buffer a kernel reads was written in full by the kernel before it.
//
// Forward, three launches:
//   1. bn_stats_kernel   workgroup s owns positions [s slice, (s + 1) slice) of the M = B H W (slice: a power of two, bt_plan) and
//                        writes (count, mean, M2) per channel.  Inside the slice the sums run on data shifted by K, per channel
//                        the median of the slice's first, middle and last value: S = sum(y - K), Q = sum((y - K)^2),
//                        mean = K + S / n, M2 = Q - S S / n.  K is one of the data and no single outlier (the corner pixel of a
//                        'same' convolution, say) can be it, so the subtraction in M2 loses (K - mean)^2 / var of the precision,
//                        a small number -- not mean^2 / var as E[y^2] - mean^2 would -- and on integer data with a power-of-two
//                        slice every step is exact.
//   2. bn_finish_kernel  one workgroup merges the slots with Chan's formula in its k-way form, in float64 and in slot order:
//                        mean = sum(n_s mean_s) / M,  M2 = sum(M2_s + n_s (mean_s - mean)^2).  It writes the saved mean and
//                        invstd = 1 / sqrt(M2 / M + eps), the tables scale = gamma invstd, shift = beta - mean scale, and updates the
//                        running statistics in place in their own dtype (running_var from the unbiased M2 / (M - 1)).
//                        A launch of its own, not merged into 3: with up to 1024 slots every workgroup of the apply launch
//                        would read up to 786 KB of partials, more than its share of the map.
//   3. bn_apply_*        v = fmaf(y, scale, shift); e = v > 0 ? v : expm1f(v); the full map, the pooled map (maximum of the four
//                        float32 e, rounded once) or both.
// Backward, three launches (the same split: two passes over the map and a one-workgroup sum between them):
//   1. bn_bwd_sums_kernel   per slot S1 = sum(dv), S2 = sum(dv xhat);  dv = g_e (v > 0 ? 1 : expf(v)), g_e = ga + [position wins
//                           its window] gp, xhat = (y - mean) invstd, v recomputed from y.
//   2. bn_bwd_finish_kernel dbeta = S1, dgamma = S2: the slots added in slot order.
//   3. bn_bwd_apply_kernel  dy = gamma invstd (dv - S1 / M - xhat S2 / M), dv recomputed, never stored.
// Pool winner: decided on the bf16 conv outputs -- the first position in the order (0,0), (0,1), (1,0), (1,1) among those with the
// largest s y, s the sign of gamma (e is monotone in s y, so this is the forward's maximum); gamma = 0: position (0,0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_bf16.h"

namespace ssdhip {
namespace {

constexpr int BT_THREADS = 256;
constexpr int BT_MAX_SLOTS = 1024;
constexpr int BT_FINISH_WAYS = 16;                       // threads per channel of the finish launches

struct BtPlan {
    int cvec;        // 16-byte lanes per pixel: C / 8
    int ppb;         // pixel lanes per workgroup: 64 (C = 32) or 32 (C = 48: 192 threads work; C = 64)
    u32 slice;       // positions per slot, a power of two
    int slots;
};

bool bt_plan(long long M, int C, BtPlan& p) {
    if (M < 2 || M > 0x7fffffffLL || (C != 32 && C != 48 && C != 64)) return false;
    p.cvec = C / 8;
    p.ppb = C == 32 ? 64 : 32;
    long long slice = 128;
    while ((M + slice - 1) / slice > BT_MAX_SLOTS) slice *= 2;
    p.slice = (u32)slice;
    p.slots = (int)((M + slice - 1) / slice);
    return true;
}

__device__ __forceinline__ void bt_unpack(const uint4 v, float (&f)[8]) {
    const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f[2 * q] = __uint_as_float(w[q] << 16);
        f[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
    }
}

__device__ __forceinline__ uint4 bt_pack(const float (&f)[8]) {
    return make_uint4(pack2_bf16(f[0], f[1]), pack2_bf16(f[2], f[3]), pack2_bf16(f[4], f[5]), pack2_bf16(f[6], f[7]));
}

// gamma / beta / a running buffer, float32 or bf16, 8 channels from c0
__device__ __forceinline__ void bt_load8(const void* p, int is_bf16, int c0, float (&f)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
        f[q] = is_bf16 ? bf16_float(static_cast<const bf16_t*>(p)[c0 + q]) : static_cast<const float*>(p)[c0 + q];
}

// red[k][tid] (k < NK) summed over the pixel lanes of each channel lane, into pixel lane 0; fixed tree
template <int NK>
__device__ __forceinline__ void bt_reduce(float* red, int tid, int pl, int cvec, int ppb) {
    __syncthreads();
    for (int s = 32; s >= 1; s >>= 1) {
        if (pl < s && pl + s < ppb) {
#pragma unroll
            for (int k = 0; k < NK; ++k) red[k * BT_THREADS + tid] += red[k * BT_THREADS + tid + s * cvec];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BT_THREADS) void bn_stats_kernel(const uint4* __restrict__ y, float* __restrict__ part, u32 M, u32 slice,
                                                              int cvec, int ppb) {
    __shared__ float red[16 * BT_THREADS];
    const int tid = threadIdx.x, cg = tid % cvec, pl = tid / cvec, C = cvec * 8;
    const u32 start = blockIdx.x * slice, end = min(M, start + slice);
    float K[8], S[8], Q[8];
    {                                                        // the shift: per channel the median of the slice's first, middle and last value
        float a[8], b[8], c[8];
        bt_unpack(y[(size_t)start * cvec + cg], a);
        bt_unpack(y[(size_t)(start + (end - start) / 2) * cvec + cg], b);
        bt_unpack(y[(size_t)(end - 1) * cvec + cg], c);
#pragma unroll
        for (int q = 0; q < 8; ++q) K[q] = fmaxf(fminf(a[q], b[q]), fminf(fmaxf(a[q], b[q]), c[q]));
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) S[q] = Q[q] = 0.f;
    if (pl < ppb) {
#pragma unroll 4
        for (u32 p = start + pl; p < end; p += ppb) {
            float f[8];
            bt_unpack(y[(size_t)p * cvec + cg], f);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float d = f[q] - K[q];
                S[q] += d;
                Q[q] += d * d;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        red[q * BT_THREADS + tid] = S[q];
        red[(8 + q) * BT_THREADS + tid] = Q[q];
    }
    bt_reduce<16>(red, tid, pl, cvec, ppb);
    if (pl == 0) {
        const float n = (float)(end - start);
        float* out = part + (size_t)blockIdx.x * 3 * C + cg * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float s = red[q * BT_THREADS + tid], qq = red[(8 + q) * BT_THREADS + tid];
            const float m2 = qq - s * s / n;
            out[q] = n;
            out[C + q] = K[q] + s / n;
            out[2 * C + q] = m2 < 0.f ? 0.f : m2;            // (a NaN stays a NaN)
        }
    }
}

__device__ __forceinline__ void bt_store_running(void* p, int is_bf16, int c, double v) {
    if (is_bf16) static_cast<bf16_t*>(p)[c] = bf16_bits<bf16_t>((float)v);
    else static_cast<float*>(p)[c] = (float)v;
}

// one workgroup of BT_FINISH_WAYS x C threads: thread (j, c) adds the slots j, j + 16, ... of channel c, thread (0, c) the 16 sums in order
__global__ __launch_bounds__(1024) void bn_finish_kernel(const float* __restrict__ part, int slots, int C, double M, const void* gamma,
                                                         const void* beta, int param_bf16, void* running_mean, void* running_var,
                                                         int running_bf16, double momentum, double eps, float* __restrict__ mean_out,
                                                         float* __restrict__ invstd_out, float* __restrict__ tables) {
    __shared__ double red[1024];
    __shared__ double mean_s[64];
    const int tid = threadIdx.x, c = tid % C, j = tid / C;
    double acc = 0.0;
    for (int s = j; s < slots; s += BT_FINISH_WAYS) acc += (double)part[(size_t)s * 3 * C + c] * (double)part[(size_t)s * 3 * C + C + c];
    red[tid] = acc;
    __syncthreads();
    if (j == 0) {
        double t = 0.0;
        for (int k = 0; k < BT_FINISH_WAYS; ++k) t += red[k * C + c];
        mean_s[c] = t / M;
    }
    __syncthreads();
    const double mean = mean_s[c];
    acc = 0.0;
    for (int s = j; s < slots; s += BT_FINISH_WAYS) {
        const float* ps = part + (size_t)s * 3 * C;
        const double d = (double)ps[C + c] - mean;
        acc += (double)ps[2 * C + c] + (double)ps[c] * d * d;
    }
    red[tid] = acc;
    __syncthreads();
    if (j == 0) {
        double m2 = 0.0;
        for (int k = 0; k < BT_FINISH_WAYS; ++k) m2 += red[k * C + c];
        const float meanf = (float)mean, invstd = (float)(1.0 / sqrt(m2 / M + eps));
        const float g = param_bf16 ? bf16_float(static_cast<const bf16_t*>(gamma)[c]) : static_cast<const float*>(gamma)[c];
        const float b = param_bf16 ? bf16_float(static_cast<const bf16_t*>(beta)[c]) : static_cast<const float*>(beta)[c];
        const float scale = g * invstd;
        mean_out[c] = meanf;
        invstd_out[c] = invstd;
        tables[c] = scale;
        tables[C + c] = b - meanf * scale;
        if (running_mean != nullptr) {
            const double rm = running_bf16 ? (double)bf16_float(static_cast<const bf16_t*>(running_mean)[c])
                                           : (double)static_cast<const float*>(running_mean)[c];
            const double rv = running_bf16 ? (double)bf16_float(static_cast<const bf16_t*>(running_var)[c])
                                           : (double)static_cast<const float*>(running_var)[c];
            bt_store_running(running_mean, running_bf16, c, (1.0 - momentum) * rm + momentum * mean);
            bt_store_running(running_var, running_bf16, c, (1.0 - momentum) * rv + momentum * (m2 / (M - 1.0)));
        }
    }
}

__device__ __forceinline__ void bt_elu8(const float (&f)[8], const float (&scale)[8], const float (&shift)[8], float (&e)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float v = fmaf(f[q], scale[q], shift[q]);
        e[q] = v > 0.f ? v : expm1f(v);
    }
}

// the full map alone: one lane per 16 bytes
__global__ __launch_bounds__(BT_THREADS) void bn_apply_full_kernel(const uint4* __restrict__ y, const float* __restrict__ tables,
                                                                   uint4* __restrict__ full, u32 M, int cvec, int ppb) {
    const int tid = threadIdx.x, cg = tid % cvec, pl = tid / cvec, C = cvec * 8;
    if (pl >= ppb) return;
    float scale[8], shift[8];
    bt_load8(tables, 0, cg * 8, scale);
    bt_load8(tables + C, 0, cg * 8, shift);
#pragma unroll 2
    for (u32 p = blockIdx.x * (u32)ppb + pl; p < M; p += gridDim.x * (u32)ppb) {
        float f[8], e[8];
        bt_unpack(y[(size_t)p * cvec + cg], f);
        bt_elu8(f, scale, shift, e);
        full[(size_t)p * cvec + cg] = bt_pack(e);
    }
}

// the pooled map [and the full one]: one lane per 8 channels of a 2 x 2 window; with KEEP the odd last column / row, which belong to
// no window, are walked behind the windows
template <bool KEEP>
__global__ __launch_bounds__(BT_THREADS) void bn_apply_pool_kernel(const uint4* __restrict__ y, const float* __restrict__ tables,
                                                                   uint4* __restrict__ full, uint4* __restrict__ pooled, int B, int H, int W,
                                                                   int cvec, int ppb) {
    const int tid = threadIdx.x, cg = tid % cvec, pl = tid / cvec, C = cvec * 8;
    if (pl >= ppb) return;
    float scale[8], shift[8];
    bt_load8(tables, 0, cg * 8, scale);
    bt_load8(tables + C, 0, cg * 8, shift);
    const u32 Ho = (u32)H / 2, Wo = (u32)W / 2, n_win = (u32)B * Ho * Wo, step = gridDim.x * (u32)ppb;
    for (u32 i = blockIdx.x * (u32)ppb + pl; i < n_win; i += step) {
        const u32 wo = i % Wo, r = i / Wo, ho = r % Ho, b = r / Ho;
        const size_t p00 = ((size_t)b * H + 2 * ho) * W + 2 * wo;
        const size_t at[4] = {p00, p00 + 1, p00 + W, p00 + W + 1};
        uint4 in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) in[k] = y[at[k] * cvec + cg];
        float m[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float f[8], e[8];
            bt_unpack(in[k], f);
            bt_elu8(f, scale, shift, e);
            if (KEEP) full[at[k] * cvec + cg] = bt_pack(e);
#pragma unroll
            for (int q = 0; q < 8; ++q) m[q] = (k == 0 || e[q] > m[q] || e[q] != e[q]) ? e[q] : m[q];     // a NaN wins, as in max_pool2d
        }
        pooled[(size_t)i * cvec + cg] = bt_pack(m);
    }
    if (KEEP) {
        const u32 n_col = (W & 1) ? (u32)B * H : 0u;                       // column W - 1 of every row
        const u32 n_row = (H & 1) ? (u32)B * (2 * Wo) : 0u;                // row H - 1, the columns in front of that one
        for (u32 i = blockIdx.x * (u32)ppb + pl; i < n_col + n_row; i += step) {
            size_t p;
            if (i < n_col) p = (size_t)i * W + (W - 1);
            else {
                const u32 k = i - n_col, b = k / (2 * Wo), w = k % (2 * Wo);
                p = ((size_t)b * H + (H - 1)) * W + w;
            }
            float f[8], e[8];
            bt_unpack(y[p * cvec + cg], f);
            bt_elu8(f, scale, shift, e);
            full[p * cvec + cg] = bt_pack(e);
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
struct BtBwd {
    const uint4* y;
    const uint4* ga;         // gradient of the full map, or null
    const uint4* gp;         // gradient of the pooled map, or null
    const float* mean;
    const float* invstd;
    const void* gamma;
    const void* beta;
    int param_bf16;
    int H, W, Ho, Wo, cvec, ppb;
    u32 M;
};

struct BtChan {              // a lane's 8 channels
    float scale[8], shift[8], mean[8], invstd[8], gamma[8];
};

__device__ __forceinline__ void bt_chan(const BtBwd& a, int cg, BtChan& t) {
    float beta[8];
    bt_load8(a.gamma, a.param_bf16, cg * 8, t.gamma);
    bt_load8(a.beta, a.param_bf16, cg * 8, beta);
    bt_load8(a.mean, 0, cg * 8, t.mean);
    bt_load8(a.invstd, 0, cg * 8, t.invstd);
#pragma unroll
    for (int q = 0; q < 8; ++q) {                                          // the forward's tables, the same operations: the same bits
        t.scale[q] = t.gamma[q] * t.invstd[q];
        t.shift[q] = beta[q] - t.mean[q] * t.scale[q];
    }
}

// dv and xhat of position p for the lane's 8 channels
__device__ __forceinline__ void bt_dv(const BtBwd& a, const BtChan& t, u32 p, int cg, float (&dv)[8], float (&xhat)[8]) {
    float f[8], g[8];
    bt_unpack(a.y[(size_t)p * a.cvec + cg], f);
    if (a.ga != nullptr) bt_unpack(a.ga[(size_t)p * a.cvec + cg], g);
    else {
#pragma unroll
        for (int q = 0; q < 8; ++q) g[q] = 0.f;
    }
    if (a.gp != nullptr) {
        const u32 w = p % (u32)a.W, r = p / (u32)a.W, h = r % (u32)a.H, b = r / (u32)a.H;
        const u32 ho = h >> 1, wo = w >> 1;
        if (ho < (u32)a.Ho && wo < (u32)a.Wo) {
            const int self = (int)((h & 1) * 2 + (w & 1));
            const size_t p00 = ((size_t)b * a.H + 2 * ho) * a.W + 2 * wo;
            const size_t at[4] = {p00, p00 + 1, p00 + a.W, p00 + a.W + 1};
            float yw[4][8], gpf[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) bt_unpack(a.y[at[k] * a.cvec + cg], yw[k]);
            bt_unpack(a.gp[(((size_t)b * a.Ho + ho) * a.Wo + wo) * a.cvec + cg], gpf);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float s = t.gamma[q] < 0.f ? -1.f : 1.f;
                int best = 0;
                float key = s * yw[0][q];
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    const float kk = s * yw[k][q];
                    if (kk > key) { key = kk; best = k; }
                }
                if (t.gamma[q] == 0.f) best = 0;
                if (best == self) g[q] += gpf[q];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float v = fmaf(f[q], t.scale[q], t.shift[q]);
        dv[q] = g[q] * (v > 0.f ? 1.f : expf(v));
        xhat[q] = (f[q] - t.mean[q]) * t.invstd[q];
    }
}

__global__ __launch_bounds__(BT_THREADS) void bn_bwd_sums_kernel(const BtBwd a, float* __restrict__ part, u32 slice) {
    __shared__ float red[16 * BT_THREADS];
    const int tid = threadIdx.x, cg = tid % a.cvec, pl = tid / a.cvec, C = a.cvec * 8;
    const u32 start = blockIdx.x * slice, end = min(a.M, start + slice);
    BtChan t;
    bt_chan(a, cg, t);
    float s1[8], s2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) s1[q] = s2[q] = 0.f;
    if (pl < a.ppb) {
        for (u32 p = start + pl; p < end; p += a.ppb) {
            float dv[8], xhat[8];
            bt_dv(a, t, p, cg, dv, xhat);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                s1[q] += dv[q];
                s2[q] += dv[q] * xhat[q];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        red[q * BT_THREADS + tid] = s1[q];
        red[(8 + q) * BT_THREADS + tid] = s2[q];
    }
    bt_reduce<16>(red, tid, pl, a.cvec, a.ppb);
    if (pl == 0) {
        float* out = part + (size_t)blockIdx.x * 2 * C + cg * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            out[q] = red[q * BT_THREADS + tid];
            out[C + q] = red[(8 + q) * BT_THREADS + tid];
        }
    }
}

// sums[0][c] = dbeta = S1, sums[1][c] = dgamma = S2: thread (j, c) adds the slots j, j + 16, ..., thread (0, c) the 16 sums in order
__global__ __launch_bounds__(1024) void bn_bwd_finish_kernel(const float* __restrict__ part, int slots, int C, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
    __shared__ double red[2][1024];
    const int tid = threadIdx.x, c = tid % C, j = tid / C;
    double a1 = 0.0, a2 = 0.0;
    for (int s = j; s < slots; s += BT_FINISH_WAYS) {
        a1 += (double)part[(size_t)s * 2 * C + c];
        a2 += (double)part[(size_t)s * 2 * C + C + c];
    }
    red[0][tid] = a1;
    red[1][tid] = a2;
    __syncthreads();
    if (j == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < BT_FINISH_WAYS; ++k) {
            t1 += red[0][k * C + c];
            t2 += red[1][k * C + c];
        }
        dbeta[c] = (float)t1;
        dgamma[c] = (float)t2;
    }
}

__global__ __launch_bounds__(BT_THREADS) void bn_bwd_apply_kernel(const BtBwd a, const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                                  uint4* __restrict__ dy) {
    const int tid = threadIdx.x, cg = tid % a.cvec, pl = tid / a.cvec;
    if (pl >= a.ppb) return;
    BtChan t;
    bt_chan(a, cg, t);
    float k1[8], k2[8];
    bt_load8(dbeta, 0, cg * 8, k1);
    bt_load8(dgamma, 0, cg * 8, k2);
    const float m = (float)a.M;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        k1[q] = k1[q] / m;
        k2[q] = k2[q] / m;
    }
    for (u32 p = blockIdx.x * (u32)a.ppb + pl; p < a.M; p += gridDim.x * (u32)a.ppb) {
        float dv[8], xhat[8], out[8];
        bt_dv(a, t, p, cg, dv, xhat);
#pragma unroll
        for (int q = 0; q < 8; ++q) out[q] = t.scale[q] * ((dv[q] - k1[q]) - xhat[q] * k2[q]);
        dy[(size_t)p * a.cvec + cg] = bt_pack(out);
    }
}

int bt_grid(long long items, int ppb) {
    long long blocks = (items + (long long)ppb * 4 - 1) / ((long long)ppb * 4);
    return (int)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
}

}  // namespace
}  // namespace ssdhip

using namespace ssdhip;

extern "C" int ssdhip_bn_elu_train_blocks(long long positions, int C) {
    BtPlan p;
    return bt_plan(positions, C, p) ? p.slots : 0;
}

extern "C" int ssdhip_bn_elu_train_fwd_nhwc_bf16(const void* y, const void* gamma, const void* beta, int param_bf16, void* running_mean,
                                                 void* running_var, int running_bf16, double momentum, double eps, void* full, void* pooled,
                                                 float* mean, float* invstd, float* tables, float* partial, int B, int H, int W, int C,
                                                 int n_slots, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    BtPlan p;
    if (!y || !gamma || !beta || !mean || !invstd || !tables || !partial || (!full && !pooled) || B <= 0 || H <= 0 || W <= 0)
        return SSDHIP_E_BADARG;
    if ((running_mean == nullptr) != (running_var == nullptr) || !(eps >= 0.0)) return SSDHIP_E_BADARG;
    const long long M = (long long)B * H * W;
    if (!bt_plan(M, C, p) || n_slots != p.slots) return SSDHIP_E_BADARG;
    if (pooled && (H < 2 || W < 2)) return SSDHIP_E_BADARG;                // no window: the pooled map would be empty
    hipLaunchKernelGGL(bn_stats_kernel, dim3(p.slots), dim3(BT_THREADS), 0, stream, static_cast<const uint4*>(y), partial, (u32)M, p.slice,
                       p.cvec, p.ppb);
    hipLaunchKernelGGL(bn_finish_kernel, dim3(1), dim3(BT_FINISH_WAYS * C), 0, stream, partial, p.slots, C, (double)M, gamma, beta,
                       param_bf16, running_mean, running_var, running_bf16, momentum, eps, mean, invstd, tables);
    if (!pooled) {
        hipLaunchKernelGGL(bn_apply_full_kernel, dim3(bt_grid(M, p.ppb)), dim3(BT_THREADS), 0, stream, static_cast<const uint4*>(y), tables,
                           static_cast<uint4*>(full), (u32)M, p.cvec, p.ppb);
    } else {
        const int grid = bt_grid((long long)B * (H / 2) * (W / 2), p.ppb);
        if (full)
            hipLaunchKernelGGL(bn_apply_pool_kernel<true>, dim3(grid), dim3(BT_THREADS), 0, stream, static_cast<const uint4*>(y), tables,
                               static_cast<uint4*>(full), static_cast<uint4*>(pooled), B, H, W, p.cvec, p.ppb);
        else
            hipLaunchKernelGGL(bn_apply_pool_kernel<false>, dim3(grid), dim3(BT_THREADS), 0, stream, static_cast<const uint4*>(y), tables,
                               static_cast<uint4*>(nullptr), static_cast<uint4*>(pooled), B, H, W, p.cvec, p.ppb);
    }
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_bn_elu_train_bwd_nhwc_bf16(const void* y, const float* mean, const float* invstd, const void* gamma, const void* beta,
                                                 int param_bf16, const void* g_full, const void* g_pooled, void* dy, float* dgamma,
                                                 float* dbeta, float* partial, int B, int H, int W, int C, int n_slots, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    BtPlan p;
    if (!y || !mean || !invstd || !gamma || !beta || (!g_full && !g_pooled) || !dy || !dgamma || !dbeta || !partial || B <= 0 || H <= 0
            || W <= 0)
        return SSDHIP_E_BADARG;
    const long long M = (long long)B * H * W;
    if (!bt_plan(M, C, p) || n_slots != p.slots) return SSDHIP_E_BADARG;
    if (g_pooled && (H < 2 || W < 2)) return SSDHIP_E_BADARG;
    BtBwd a;
    a.y = static_cast<const uint4*>(y);
    a.ga = static_cast<const uint4*>(g_full);
    a.gp = static_cast<const uint4*>(g_pooled);
    a.mean = mean;
    a.invstd = invstd;
    a.gamma = gamma;
    a.beta = beta;
    a.param_bf16 = param_bf16;
    a.H = H;
    a.W = W;
    a.Ho = H / 2;
    a.Wo = W / 2;
    a.cvec = p.cvec;
    a.ppb = p.ppb;
    a.M = (u32)M;
    hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(p.slots), dim3(BT_THREADS), 0, stream, a, partial, p.slice);
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(1), dim3(BT_FINISH_WAYS * C), 0, stream, partial, p.slots, C, dgamma, dbeta);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(bt_grid(M, p.ppb)), dim3(BT_THREADS), 0, stream, a, dgamma, dbeta, static_cast<uint4*>(dy));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
