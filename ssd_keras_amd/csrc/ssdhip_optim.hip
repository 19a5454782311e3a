// ssdhip_optim.hip -- the parameter side of the TRAINING step on gfx950 (MI355X): one launch over ALL parameters instead of one or
// two framework kernels per layer.
//
// The reference trains with keras.optimizers.SGD(lr=0.001, momentum=0.9) on float32 weights (ssd300_training.ipynb:169-173).  Here the
// float32 master weights stay the optimizer's; what the MFMA kernels read are bf16 copies in the layouts they want:
//   * the layer's filters [Cout][kh][kw][Cin] bf16 (channels_last) for the forward pass and the weight gradient,
//   * the same filters transposed (Cin <-> Cout) with their taps flipped, [Cin][kh][kw][Cout], for the data gradient (a stride-1 'same'
//     convolution of dL/dy with exactly those filters).
// Round 4 built them per layer and per step with framework ops: a cast, a layout copy where a kernel wanted channels_last, torch.flip +
// permute + contiguous in every backward, torch.cat for the packed predictor heads -- 52 copies, 19 flips, 15 concatenations, 24 fills:
// ~0.8 ms and ~110 launches of an 11 ms step (profiles/r05h_train_step_timeline.json).
//
//   shadow_refresh_kernel   grid = tiles of 32 x 32 (Cout x Cin) filter taps over every weight tensor + a tail for the 1-D tensors
//                           (biases, L2Normalization's gamma): float32 master -> bf16 through LDS, both layouts written as 64-byte runs.
//   sgd_momentum_kernel     torch.optim.SGD's update (buf = momentum buf + g [+ wd p]; p -= lr buf; the first step's buf = g), every
//                           parameter in one launch, float32.  `lr` is a kernel argument: a captured launch replays it.
//   sgd_tick_kernel / sgd_step_kernel<RULE, NESTEROV>
//                           the same launch shape with its scalars in a state block on the DEVICE, as Adam's (ssdhip_adam.hip): a
//                           one-workgroup tick advances `iterations` and rounds lr_t = lr0 / (1 + decay (iterations - 1)) once to float32,
//                           the update reads lr_t, momentum and weight_decay from the block -- a captured step follows ssdhip_sgd_set_lr
//                           between replays (ssd300_training.ipynb's LearningRateScheduler).  RULE 0: torch's buffer, RULE 1: Keras 2.x
//                           SGD.get_updates' velocity (v = momentum v - lr g; p += v), each with and without Nesterov.  20 bytes per
//                           parameter, as sgd_momentum_kernel.
//   sgd_step_bf16_kernel<RULE, NESTEROV>
//                           the same update (sgd_update) on a float32 MASTER copy of a bf16 parameter: bf16 gradient in (exact in
//                           float32), weight decay on the master, p = bf16(master) out, round to nearest even, never read.  Eight values
//                           per thread and pass; 20 bytes per parameter as well (2 + 8 + 8 + 2).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_math.h"
#include "ssdhip_bf16.h"

namespace ssdhip {

constexpr int SH_T = 32;                                  // tile edge (output x input channels)
constexpr int SH_MAXKK = 16;                              // taps of a filter: 1 x 1, 3 x 3, 4 x 4 (SSD512's conv10_2)

// One block = one (32 Cout x 32 Cin) tile of one weight tensor, or one 256-element run of a 1-D tensor.
__global__ __launch_bounds__(256) void shadow_refresh_kernel(const ssdhip_shadow_desc* __restrict__ tab, int n_w, int n_tiles, int n_v) {
    __shared__ unsigned short tile[SH_MAXKK * SH_T * (SH_T + 2)];
    __shared__ int sh_which;
    const int tid = threadIdx.x;
    int blk = (int)blockIdx.x;
    if (blk >= n_tiles) {                                 // ---- 1-D tensors: descriptors n_w .. n_w + n_v - 1, tile0 = first run
        blk -= n_tiles;
        if (tid == 0) {
            int k = n_w;
            while (k + 1 < n_w + n_v && tab[k + 1].tile0 <= blk) ++k;
            sh_which = k;
        }
        __syncthreads();
        const ssdhip_shadow_desc d = tab[sh_which];
        const int i = (blk - d.tile0) * 256 + tid;
        if (i < d.O) static_cast<unsigned short*>(d.cl)[i] = bf16_bits<bf16_t>(static_cast<const float*>(d.src)[i]);
        return;
    }
    if (tid == 0) {
        int k = 0;
        while (k + 1 < n_w && tab[k + 1].tile0 <= blk) ++k;
        sh_which = k;
    }
    __syncthreads();
    const ssdhip_shadow_desc d = tab[sh_which];
    const int kk = d.KK;
    const int ti = (d.I + SH_T - 1) / SH_T;
    const int t = blk - d.tile0;
    const int o0 = (t / ti) * SH_T, i0 = (t % ti) * SH_T;
    const int no = min(SH_T, d.O - o0), ni = min(SH_T, d.I - i0);
    const float* src = static_cast<const float*>(d.src);
    const int run = ni * kk;
    // (six loads in flight per thread and trip: one at a time, a tile of 9216 values was 36 dependent memory round trips per workgroup
    //  and the launch ran at a third of the HBM rate)
    constexpr int SH_U = 6;
    const int n_el = no * run;
    if (d.src_channels_last) {
        // master [O][kk][I] float32 (a channels_last parameter): runs of ni values per (o, tap)
        for (int e0 = tid; e0 < n_el; e0 += 256 * SH_U) {
            float v[SH_U];
            int at[SH_U];
#pragma unroll
            for (int u = 0; u < SH_U; ++u) {
                const int e = e0 + 256 * u, ec = e < n_el ? e : 0;
                const int o = ec / run, j = ec - o * run;
                const int tap = j / ni, i = j - tap * ni;
                at[u] = e < n_el ? (tap * SH_T + o) * (SH_T + 2) + i : -1;
                v[u] = src[((size_t)(o0 + o) * kk + tap) * d.I + i0 + i];
            }
#pragma unroll
            for (int u = 0; u < SH_U; ++u)
                if (at[u] >= 0) tile[at[u]] = bf16_bits<bf16_t>(v[u]);
        }
    } else {
        // master [O][I][kk] float32: the tile's row o is the contiguous run [i0 .. i0 + ni) x kk
        for (int e0 = tid; e0 < n_el; e0 += 256 * SH_U) {
            float v[SH_U];
            int at[SH_U];
#pragma unroll
            for (int u = 0; u < SH_U; ++u) {
                const int e = e0 + 256 * u, ec = e < n_el ? e : 0;
                const int o = ec / run, j = ec - o * run;
                const int i = j / kk, tap = j - i * kk;
                at[u] = e < n_el ? (tap * SH_T + o) * (SH_T + 2) + i : -1;
                v[u] = src[((size_t)(o0 + o) * d.I + i0) * kk + j];
            }
#pragma unroll
            for (int u = 0; u < SH_U; ++u)
                if (at[u] >= 0) tile[at[u]] = bf16_bits<bf16_t>(v[u]);
        }
    }
    __syncthreads();
    // channels_last copy [O][kk][I]: runs of ni values
    // (four values = 8 bytes per store where the runs allow it: two-byte stores left the launch at 1.6 TB/s)
    unsigned short* cl = static_cast<unsigned short*>(d.cl);
    if (cl) {
        if (!(d.I & 3) && !((uintptr_t)cl & 7)) {                       // i0 is a multiple of 32, so ni % 4 == 0 as well
            for (int e = tid; e < no * kk * (SH_T / 4); e += 256) {
                const int i = (e & (SH_T / 4 - 1)) * 4, r = e >> 3;
                const int tap = r % kk, o = r / kk;
                if (i < ni) {
                    const u32* t2 = reinterpret_cast<const u32*>(&tile[(tap * SH_T + o) * (SH_T + 2) + i]);   // rows are 68 bytes: 4-byte aligned
                    *reinterpret_cast<uint2*>(&cl[((size_t)(o0 + o) * kk + tap) * d.I + i0 + i]) = make_uint2(t2[0], t2[1]);
                }
            }
        } else {
            for (int e = tid; e < no * kk * SH_T; e += 256) {
                const int i = e & (SH_T - 1), r = e >> 5;
                const int tap = r % kk, o = r / kk;
                if (i < ni) cl[((size_t)(o0 + o) * kk + tap) * d.I + i0 + i] = tile[(tap * SH_T + o) * (SH_T + 2) + i];
            }
        }
    }
    // transposed, taps flipped [I][kk][tr_ostride] at channel offset tr_ooff: runs of no values
    unsigned short* tr = static_cast<unsigned short*>(d.tr);
    if (tr) {
        if (!(d.tr_ostride & 3) && !(d.tr_ooff & 3) && !(no & 3) && !((uintptr_t)tr & 7)) {
            for (int e = tid; e < ni * kk * (SH_T / 4); e += 256) {
                const int o = (e & (SH_T / 4 - 1)) * 4, r = e >> 3;
                const int tap = r % kk, i = r / kk;
                if (o < no) {
                    const unsigned short* tp = &tile[(tap * SH_T + o) * (SH_T + 2) + i];
                    const u32 a = tp[0], b = tp[SH_T + 2], c = tp[2 * (SH_T + 2)], e3 = tp[3 * (SH_T + 2)];
                    *reinterpret_cast<uint2*>(&tr[((size_t)(i0 + i) * kk + (kk - 1 - tap)) * d.tr_ostride + d.tr_ooff + o0 + o]) =
                        make_uint2(a | (b << 16), c | (e3 << 16));
                }
            }
        } else {
            for (int e = tid; e < ni * kk * SH_T; e += 256) {
                const int o = e & (SH_T - 1), r = e >> 5;
                const int tap = r % kk, i = r / kk;
                if (o < no) tr[((size_t)(i0 + i) * kk + (kk - 1 - tap)) * d.tr_ostride + d.tr_ooff + o0 + o] = tile[(tap * SH_T + o) * (SH_T + 2) + i];
            }
        }
    }
}

// torch.optim.SGD (momentum, dampening 0, no Nesterov): four values per thread and step, up to SGD_CHUNK tensors per launch.  The
// tensor table travels in the KERNEL ARGUMENTS: gradients are new tensors every step (zero_grad(set_to_none=True)), and a device-side
// table would have to be re-uploaded -- a pageable host-to-device copy that blocks the host until the whole backward pass has drained
// (measured: the step 0.3-0.5 ms SLOWER than with the framework's optimizer although the kernels took 250 us less).
constexpr int SGD_CHUNK = 80;
struct SgdArgs {
    float* p[SGD_CHUNK];
    const float* g[SGD_CHUNK];
    float* m[SGD_CHUNK];
    long long n[SGD_CHUNK];
    int block0[SGD_CHUNK];                                 // first block of each tensor (4096 values per block)
    int count;
};

__global__ __launch_bounds__(256) void sgd_momentum_kernel(const SgdArgs a, float lr, float momentum, float weight_decay) {
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    int lo = 0, hi = a.count - 1;                          // last tensor with block0 <= blk (uniform: scalar loads of the arguments)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    float* p = a.p[lo];
    const float* g = a.g[lo];
    float* m = a.m[lo];
    const long long n = a.n[lo];
    const long long base = (long long)(blk - a.block0[lo]) * 4096;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long i = base + (long long)u * 1024 + tid * 4;
        if (i + 3 < n) {
            const float4 pv = *reinterpret_cast<const float4*>(p + i), gv = *reinterpret_cast<const float4*>(g + i);
            const float4 mv = *reinterpret_cast<const float4*>(m + i);
            float gg[4] = {gv.x, gv.y, gv.z, gv.w}, pp[4] = {pv.x, pv.y, pv.z, pv.w}, mm[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float gq = gg[q];
                if (weight_decay != 0.f) gq = gq + weight_decay * pp[q];
                mm[q] = momentum * mm[q] + gq;
                pp[q] = pp[q] - lr * mm[q];
            }
            *reinterpret_cast<float4*>(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *reinterpret_cast<float4*>(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
        } else {
            for (long long j = i; j < n && j < i + 4; ++j) {
                float gq = g[j];
                if (weight_decay != 0.f) gq = gq + weight_decay * p[j];
                const float mq = momentum * m[j] + gq;
                m[j] = mq;
                p[j] = p[j] - lr * mq;
            }
        }
    }
}

__global__ __launch_bounds__(64) void sgd_init_kernel(ssdhip_sgd_state* st, int n_groups, int group, double lr, double momentum,
                                                      double decay, double weight_decay, long long iterations) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->iterations = iterations;                           // (every group's call rewrites the same count)
    st->n_groups = n_groups;
    st->reserved = 0;
    ssdhip_sgd_group& s = st->groups[group];
    s.lr = lr;
    s.decay = decay;
    s.momentum = momentum;
    s.lr_t = 0.f;                                          // (the tick in front of every update writes it)
    s.momentum_f = (float)momentum;
    s.weight_decay = (float)weight_decay;
    s.reserved = 0;
}

__global__ __launch_bounds__(64) void sgd_set_lr_kernel(ssdhip_sgd_state* st, int group, double lr) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && group < st->n_groups) st->groups[group].lr = lr;
}

// One workgroup, one thread per parameter group.
__global__ __launch_bounds__(SSDHIP_ADAM_MAX_GROUPS) void sgd_tick_kernel(ssdhip_sgd_state* st) {
    const int g = threadIdx.x;
    const long long t = st->iterations + 1;
    const int n_groups = st->n_groups;
    __syncthreads();                                       // every thread has read the old count
    if (g == 0) st->iterations = t;
    if (g >= n_groups) return;
    ssdhip_sgd_group& s = st->groups[g];
    double lr = s.lr;
    if (s.decay > 0.0) lr = lr / (1.0 + s.decay * (double)(t - 1));   // Keras reads `iterations` before it increments it
    s.lr_t = (float)lr;
}

// One element of the update; `m` is the momentum buffer (RULE 0) or the velocity (RULE 1).  One IEEE float32 operation per line part,
// in the order of include/ssdhip.h; RULE 0 without Nesterov is sgd_momentum_kernel's sequence.
template <int RULE, bool NESTEROV>
__device__ __forceinline__ void sgd_update(float& p, float g, float& m, float lr, float momentum, float weight_decay) {
    if (weight_decay != 0.f) g = g + weight_decay * p;
    if (RULE == 0) {
        m = momentum * m + g;
        if (NESTEROV) {
            const float d = g + momentum * m;
            p = p - lr * d;
        } else {
            p = p - lr * m;
        }
    } else {
        const float lg = lr * g;
        m = momentum * m - lg;
        if (NESTEROV)
            p = (p + momentum * m) - lg;
        else
            p = p + m;
    }
}

template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdArgs a, const ssdhip_sgd_state* __restrict__ st, int group) {
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    if (group >= st->n_groups) return;
    const ssdhip_sgd_group& s = st->groups[group];         // uniform: scalar loads, the values the tick has just written
    const float lr = s.lr_t, momentum = s.momentum_f, weight_decay = s.weight_decay;
    int lo = 0, hi = a.count - 1;                          // last tensor with block0 <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    float* p = a.p[lo];
    const float* g = a.g[lo];
    float* m = a.m[lo];
    const long long n = a.n[lo];
    const long long base = (long long)(blk - a.block0[lo]) * 4096;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long i = base + (long long)u * 1024 + tid * 4;
        if (i + 3 < n) {
            const float4 pv = *reinterpret_cast<const float4*>(p + i), gv = *reinterpret_cast<const float4*>(g + i);
            const float4 mv = *reinterpret_cast<const float4*>(m + i);
            float gg[4] = {gv.x, gv.y, gv.z, gv.w}, pp[4] = {pv.x, pv.y, pv.z, pv.w}, mm[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) sgd_update<RULE, NESTEROV>(pp[q], gg[q], mm[q], lr, momentum, weight_decay);
            *reinterpret_cast<float4*>(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *reinterpret_cast<float4*>(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
        } else {
            for (long long j = i; j < n && j < i + 4; ++j) {
                float pq = p[j], mq = m[j];
                sgd_update<RULE, NESTEROV>(pq, g[j], mq, lr, momentum, weight_decay);
                m[j] = mq;
                p[j] = pq;
            }
        }
    }
}
static_assert(sizeof(SgdArgs) + sizeof(void*) + 2 * sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");

// Four pointers + count + first block = 44 bytes per tensor: 80 tensors are 3524 bytes.
constexpr int SGD_BF16_CHUNK = 80;
struct SgdBf16Args {
    bf16_t* p[SGD_BF16_CHUNK];                             // written only
    const bf16_t* g[SGD_BF16_CHUNK];
    float* w[SGD_BF16_CHUNK];                              // the float32 master
    float* m[SGD_BF16_CHUNK];
    long long n[SGD_BF16_CHUNK];
    int block0[SGD_BF16_CHUNK];
    int count;
};
static_assert(sizeof(SgdBf16Args) + sizeof(void*) + 2 * sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");

template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_step_bf16_kernel(const SgdBf16Args a, const ssdhip_sgd_state* __restrict__ st, int group) {
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    if (group >= st->n_groups) return;
    const ssdhip_sgd_group& s = st->groups[group];         // uniform: scalar loads, the values the tick has just written
    const float lr = s.lr_t, momentum = s.momentum_f, weight_decay = s.weight_decay;
    int lo = 0, hi = a.count - 1;                          // last tensor with block0 <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    bf16_t* p = a.p[lo];
    const bf16_t* g = a.g[lo];
    float* w = a.w[lo];
    float* m = a.m[lo];
    const long long n = a.n[lo];
    const long long base = (long long)(blk - a.block0[lo]) * 4096;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long long i = base + (long long)u * 2048 + tid * 8;
        if (i + 7 < n) {
            const uint4 gv = *reinterpret_cast<const uint4*>(g + i);
            const u32 gw[4] = {gv.x, gv.y, gv.z, gv.w};
            float ww[8], mm[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 wv = *reinterpret_cast<const float4*>(w + i + 4 * h), mv = *reinterpret_cast<const float4*>(m + i + 4 * h);
                ww[4 * h] = wv.x, ww[4 * h + 1] = wv.y, ww[4 * h + 2] = wv.z, ww[4 * h + 3] = wv.w;
                mm[4 * h] = mv.x, mm[4 * h + 1] = mv.y, mm[4 * h + 2] = mv.z, mm[4 * h + 3] = mv.w;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float gq = (q & 1) ? __uint_as_float(gw[q >> 1] & 0xffff0000u) : bf16_float(gw[q >> 1] & 0xffffu);
                sgd_update<RULE, NESTEROV>(ww[q], gq, mm[q], lr, momentum, weight_decay);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                *reinterpret_cast<float4*>(w + i + 4 * h) = make_float4(ww[4 * h], ww[4 * h + 1], ww[4 * h + 2], ww[4 * h + 3]);
                *reinterpret_cast<float4*>(m + i + 4 * h) = make_float4(mm[4 * h], mm[4 * h + 1], mm[4 * h + 2], mm[4 * h + 3]);
            }
            *reinterpret_cast<uint4*>(p + i) = make_uint4(pack2_bf16(ww[0], ww[1]), pack2_bf16(ww[2], ww[3]), pack2_bf16(ww[4], ww[5]),
                                                          pack2_bf16(ww[6], ww[7]));
        } else {
            for (long long j = i; j < n && j < i + 8; ++j) {
                float wq = w[j], mq = m[j];
                sgd_update<RULE, NESTEROV>(wq, bf16_float(g[j]), mq, lr, momentum, weight_decay);
                m[j] = mq;
                w[j] = wq;
                p[j] = bf16_bits<bf16_t>(wq);
            }
        }
    }
}

}  // namespace ssdhip

using namespace ssdhip;

extern "C" int ssdhip_shadow_refresh(const ssdhip_shadow_desc* table_dev, int n_weights, int n_tiles, int n_vectors, int n_vector_blocks,
                                     void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!table_dev || n_weights < 0 || n_vectors < 0 || n_tiles < 0 || n_vector_blocks < 0 || (n_weights == 0) != (n_tiles == 0)
        || (n_vectors == 0) != (n_vector_blocks == 0))
        return SSDHIP_E_BADARG;
    if (n_tiles + n_vector_blocks == 0) return SSDHIP_OK;
    hipLaunchKernelGGL(shadow_refresh_kernel, dim3((unsigned)(n_tiles + n_vector_blocks)), dim3(256), 0, stream, table_dev, n_weights,
                       n_tiles, n_vectors);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_sgd_momentum_step(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* bufs_h,
                                        const long long* numel_h, double lr, double momentum, double weight_decay, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_tensors <= 0 || !params_h || !grads_h || !bufs_h || !numel_h) return SSDHIP_E_BADARG;
    for (int k = 0; k < n_tensors; ++k) {
        if (!params_h[k] || !grads_h[k] || !bufs_h[k] || numel_h[k] <= 0) return SSDHIP_E_BADARG;
        if (((uintptr_t)params_h[k] | (uintptr_t)grads_h[k] | (uintptr_t)bufs_h[k]) & 15) return SSDHIP_E_BADARG;
        if ((numel_h[k] + 4095) / 4096 > 0x3fffffffLL) return SSDHIP_E_BADARG;
    }
    for (int k0 = 0; k0 < n_tensors; k0 += SGD_CHUNK) {
        SgdArgs a;
        a.count = n_tensors - k0 < SGD_CHUNK ? n_tensors - k0 : SGD_CHUNK;
        long long blocks = 0;
        for (int k = 0; k < SGD_CHUNK; ++k) {
            const int src = k < a.count ? k0 + k : k0;     // (unused slots repeat the first tensor: never selected)
            a.p[k] = static_cast<float*>(params_h[src]);
            a.g[k] = static_cast<const float*>(grads_h[src]);
            a.m[k] = static_cast<float*>(bufs_h[src]);
            a.n[k] = numel_h[src];
            a.block0[k] = (int)blocks;
            if (k < a.count) blocks += (numel_h[src] + 4095) / 4096;
            if (blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
        }
        hipLaunchKernelGGL(sgd_momentum_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a, (float)lr, (float)momentum, (float)weight_decay);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    return SSDHIP_OK;
}

extern "C" size_t ssdhip_sgd_state_bytes(int n_groups) {
    if (n_groups <= 0 || n_groups > SSDHIP_ADAM_MAX_GROUPS) return 0;
    return sizeof(ssdhip_sgd_state) + (size_t)n_groups * sizeof(ssdhip_sgd_group);
}

extern "C" int ssdhip_sgd_state_init(void* state, int n_groups, int group, double lr, double momentum, double decay, double weight_decay,
                                     long long iterations, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || n_groups <= 0 || n_groups > SSDHIP_ADAM_MAX_GROUPS || group < 0 || group >= n_groups)
        return SSDHIP_E_BADARG;
    if (!(lr >= 0.0) || !(momentum >= 0.0) || !(decay >= 0.0) || !(weight_decay >= 0.0) || iterations < 0) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(sgd_init_kernel, dim3(1), dim3(64), 0, stream, static_cast<ssdhip_sgd_state*>(state), n_groups, group, lr,
                       momentum, decay, weight_decay, iterations);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_sgd_set_lr(void* state, int group, double lr, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || group < 0 || group >= SSDHIP_ADAM_MAX_GROUPS || !(lr >= 0.0)) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(sgd_set_lr_kernel, dim3(1), dim3(64), 0, stream, static_cast<ssdhip_sgd_state*>(state), group, lr);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_sgd_step(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* bufs_h,
                               const long long* numel_h, int group, void* state, int rule, int nesterov, int tick, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_tensors <= 0 || !params_h || !grads_h || !bufs_h || !numel_h || !state || ((uintptr_t)state & 15) || group < 0
        || group >= SSDHIP_ADAM_MAX_GROUPS || rule < 0 || rule > 1)
        return SSDHIP_E_BADARG;
    for (int k = 0; k < n_tensors; ++k) {
        if (!params_h[k] || !grads_h[k] || !bufs_h[k] || numel_h[k] <= 0) return SSDHIP_E_BADARG;
        if (((uintptr_t)params_h[k] | (uintptr_t)grads_h[k] | (uintptr_t)bufs_h[k]) & 15) return SSDHIP_E_BADARG;
        if ((numel_h[k] + 4095) / 4096 > 0x3fffffffLL) return SSDHIP_E_BADARG;
    }
    ssdhip_sgd_state* st = static_cast<ssdhip_sgd_state*>(state);
    if (tick) {
        hipLaunchKernelGGL(sgd_tick_kernel, dim3(1), dim3(SSDHIP_ADAM_MAX_GROUPS), 0, stream, st);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    for (int k0 = 0; k0 < n_tensors; k0 += SGD_CHUNK) {
        SgdArgs a;
        a.count = n_tensors - k0 < SGD_CHUNK ? n_tensors - k0 : SGD_CHUNK;
        long long blocks = 0;
        for (int k = 0; k < SGD_CHUNK; ++k) {
            const int src = k < a.count ? k0 + k : k0;     // (unused slots repeat the first tensor: never selected)
            a.p[k] = static_cast<float*>(params_h[src]);
            a.g[k] = static_cast<const float*>(grads_h[src]);
            a.m[k] = static_cast<float*>(bufs_h[src]);
            a.n[k] = numel_h[src];
            a.block0[k] = (int)blocks;
            if (k < a.count) blocks += (numel_h[src] + 4095) / 4096;
            if (blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
        }
        const dim3 grid((unsigned)blocks), wg(256);
        if (rule == 0 && !nesterov)
            hipLaunchKernelGGL((sgd_step_kernel<0, false>), grid, wg, 0, stream, a, st, group);
        else if (rule == 0)
            hipLaunchKernelGGL((sgd_step_kernel<0, true>), grid, wg, 0, stream, a, st, group);
        else if (!nesterov)
            hipLaunchKernelGGL((sgd_step_kernel<1, false>), grid, wg, 0, stream, a, st, group);
        else
            hipLaunchKernelGGL((sgd_step_kernel<1, true>), grid, wg, 0, stream, a, st, group);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    return SSDHIP_OK;
}

extern "C" int ssdhip_sgd_step_bf16(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* master_h,
                                    void* const* bufs_h, const long long* numel_h, int group, void* state, int rule, int nesterov,
                                    int tick, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_tensors <= 0 || !params_h || !grads_h || !master_h || !bufs_h || !numel_h || !state || ((uintptr_t)state & 15) || group < 0
        || group >= SSDHIP_ADAM_MAX_GROUPS || rule < 0 || rule > 1)
        return SSDHIP_E_BADARG;
    long long chunk_blocks = 0;
    for (int k = 0; k < n_tensors; ++k) {
        if (!params_h[k] || !grads_h[k] || !master_h[k] || !bufs_h[k] || numel_h[k] <= 0) return SSDHIP_E_BADARG;
        if (((uintptr_t)params_h[k] | (uintptr_t)grads_h[k] | (uintptr_t)master_h[k] | (uintptr_t)bufs_h[k]) & 15) return SSDHIP_E_BADARG;
        if ((numel_h[k] + 4095) / 4096 > 0x3fffffffLL) return SSDHIP_E_BADARG;
        if (k % SGD_BF16_CHUNK == 0) chunk_blocks = 0;      // (a launch's grid, before the tick: nothing runs on a refused call)
        chunk_blocks += (numel_h[k] + 4095) / 4096;
        if (chunk_blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
    }
    ssdhip_sgd_state* st = static_cast<ssdhip_sgd_state*>(state);
    if (tick) {
        hipLaunchKernelGGL(sgd_tick_kernel, dim3(1), dim3(SSDHIP_ADAM_MAX_GROUPS), 0, stream, st);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    for (int k0 = 0; k0 < n_tensors; k0 += SGD_BF16_CHUNK) {
        SgdBf16Args a;
        a.count = n_tensors - k0 < SGD_BF16_CHUNK ? n_tensors - k0 : SGD_BF16_CHUNK;
        long long blocks = 0;
        for (int k = 0; k < SGD_BF16_CHUNK; ++k) {
            const int src = k < a.count ? k0 + k : k0;     // (unused slots repeat the first tensor: never selected)
            a.p[k] = static_cast<bf16_t*>(params_h[src]);
            a.g[k] = static_cast<const bf16_t*>(grads_h[src]);
            a.w[k] = static_cast<float*>(master_h[src]);
            a.m[k] = static_cast<float*>(bufs_h[src]);
            a.n[k] = numel_h[src];
            a.block0[k] = (int)blocks;
            if (k < a.count) blocks += (numel_h[src] + 4095) / 4096;
        }
        const dim3 grid((unsigned)blocks), wg(256);
        if (rule == 0 && !nesterov)
            hipLaunchKernelGGL((sgd_step_bf16_kernel<0, false>), grid, wg, 0, stream, a, st, group);
        else if (rule == 0)
            hipLaunchKernelGGL((sgd_step_bf16_kernel<0, true>), grid, wg, 0, stream, a, st, group);
        else if (!nesterov)
            hipLaunchKernelGGL((sgd_step_bf16_kernel<1, false>), grid, wg, 0, stream, a, st, group);
        else
            hipLaunchKernelGGL((sgd_step_bf16_kernel<1, true>), grid, wg, 0, stream, a, st, group);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    return SSDHIP_OK;
}
