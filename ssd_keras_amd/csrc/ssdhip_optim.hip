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
//   SgdRule<RULE, NESTEROV> one element of the SGD update.  RULE 0: torch.optim.SGD's buffer (buf = momentum buf + g [+ wd p]; p -= lr buf;
//                           the first step's buf = g), RULE 1: Keras 2.x SGD.get_updates' velocity (v = momentum v - lr g; p += v), each
//                           with and without Nesterov.  The three step kernels below are this rule in the ONE update body every
//                           optimizer kernel shares (optim_step, ssdhip_optim_step.h: the tensor table in the kernel arguments, 4096
//                           values per block, vector passes with a scalar tail); they differ in where the scalars come from and in the
//                           parameter's type.  20 bytes per parameter in all three.
//   sgd_momentum_kernel     SgdRule<0, false> over every float32 parameter in one launch.  `lr`, `momentum` and `weight_decay` are kernel
//                           arguments: a captured launch replays them.
//   sgd_tick_kernel / sgd_step_kernel<RULE, NESTEROV>
//                           the scalars in a state block on the DEVICE, as Adam's (ssdhip_adam.hip): a one-workgroup tick advances
//                           `iterations` and rounds lr_t = lr0 / (1 + decay (iterations - 1)) once to float32, the update reads lr_t,
//                           momentum and weight_decay from the block -- a captured step follows ssdhip_sgd_set_lr between replays
//                           (ssd300_training.ipynb's LearningRateScheduler).
//   sgd_step_bf16_kernel<RULE, NESTEROV>
//                           the same on a float32 MASTER copy of a bf16 parameter (optim_step's BF16 form: 2 + 8 + 8 + 2 bytes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_math.h"
#include "ssdhip_bf16.h"
#include "ssdhip_optim_step.h"

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

// One element of the update; `m` is the momentum buffer (RULE 0) or the velocity (RULE 1).  One IEEE float32 operation per line part,
// in the order of include/ssdhip.h; RULE 0 without Nesterov is torch.optim.SGD's (momentum, dampening 0), sgd_momentum_kernel's.
template <int RULE, bool NESTEROV>
struct SgdRule {
    static constexpr int NBUF = 1;
    struct Scalars { float lr, momentum, weight_decay; };
    static __device__ __forceinline__ void update(float& p, float g, float* m, const Scalars& c) {
        if (c.weight_decay != 0.f) g = g + c.weight_decay * p;
        if (RULE == 0) {
            m[0] = c.momentum * m[0] + g;
            if (NESTEROV) {
                const float d = g + c.momentum * m[0];
                p = p - c.lr * d;
            } else {
                p = p - c.lr * m[0];
            }
        } else {
            const float lg = c.lr * g;
            m[0] = c.momentum * m[0] - lg;
            if (NESTEROV)
                p = (p + c.momentum * m[0]) - lg;
            else
                p = p + m[0];
        }
    }
};

// 80 tensors per launch: three pointers (four with a master) + count + first block = 36 (44) bytes per tensor, 3524 bytes at most.
constexpr int SGD_CHUNK = 80;
typedef OptimTable<3, SGD_CHUNK> SgdArgs;                  // p, g, buffer
typedef OptimTable<4, SGD_CHUNK> SgdBf16Args;              // p (written only), g, master, buffer
static_assert(sizeof(SgdBf16Args) + sizeof(void*) + 2 * sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");
static_assert(sizeof(SgdArgs) + 3 * sizeof(float) <= 4096, "the tensor table must fit the kernel arguments");

__global__ __launch_bounds__(256) void sgd_momentum_kernel(const SgdArgs a, float lr, float momentum, float weight_decay) {
    optim_step<SgdRule<0, false>, false>(a, {lr, momentum, weight_decay});
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

// One workgroup, one thread per parameter group.
__device__ __forceinline__ void sgd_tick(ssdhip_sgd_state* st) {
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

__global__ __launch_bounds__(SSDHIP_ADAM_MAX_GROUPS) void sgd_tick_kernel(ssdhip_sgd_state* st) { sgd_tick(st); }

// The tick of a clipped step: a skipped step (ssdhip_clip_finish's decision) leaves the block as it is.
__global__ __launch_bounds__(SSDHIP_ADAM_MAX_GROUPS) void sgd_tick_clipped_kernel(ssdhip_sgd_state* st, const ssdhip_clip_state* clip) {
    if (clip->skip) return;
    sgd_tick(st);
}

// The state-block forms: the group's scalars are the values the tick has just written (uniform: scalar loads).
template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdArgs a, const ssdhip_sgd_state* __restrict__ st, int group) {
    if (group >= st->n_groups) return;
    const ssdhip_sgd_group& s = st->groups[group];
    optim_step<SgdRule<RULE, NESTEROV>, false>(a, {s.lr_t, s.momentum_f, s.weight_decay});
}

template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_step_bf16_kernel(const SgdBf16Args a, const ssdhip_sgd_state* __restrict__ st, int group) {
    if (group >= st->n_groups) return;
    const ssdhip_sgd_group& s = st->groups[group];
    optim_step<SgdRule<RULE, NESTEROV>, true>(a, {s.lr_t, s.momentum_f, s.weight_decay});
}

// The clipped forms: the same two kernels with Clipped<SgdRule> as their rule, nothing at all on a skipped step.
static_assert(sizeof(SgdBf16Args) + 2 * sizeof(void*) + sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");

template <int RULE, bool NESTEROV, bool BF16, class Table>
__device__ __forceinline__ void sgd_step_clipped(const Table& a, const ssdhip_sgd_state* __restrict__ st, int group,
                                                 const ssdhip_clip_state* __restrict__ clip) {
    if (group >= st->n_groups || clip->skip) return;
    const ssdhip_sgd_group& s = st->groups[group];
    optim_step<Clipped<SgdRule<RULE, NESTEROV>>, BF16>(a, {{s.lr_t, s.momentum_f, 0.f}, s.weight_decay, clip});
}

template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_step_clipped_kernel(const SgdArgs a, const ssdhip_sgd_state* __restrict__ st, int group,
                                                               const ssdhip_clip_state* __restrict__ clip) {
    sgd_step_clipped<RULE, NESTEROV, false>(a, st, group, clip);
}

template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_step_bf16_clipped_kernel(const SgdBf16Args a, const ssdhip_sgd_state* __restrict__ st, int group,
                                                                    const ssdhip_clip_state* __restrict__ clip) {
    sgd_step_clipped<RULE, NESTEROV, true>(a, st, group, clip);
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
    return optim_launch<SGD_CHUNK>(static_cast<hipStream_t>(stream_), n_tensors, {params_h, grads_h, bufs_h}, numel_h, [] { return true; },
                                   sgd_momentum_kernel, (float)lr, (float)momentum, (float)weight_decay);
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
    return optim_set_lr<ssdhip_sgd_state>(state, group, lr, stream_);
}

#define SGD_PICK(K, rule, nesterov) ((rule) ? ((nesterov) ? K<1, true> : K<1, false>) : ((nesterov) ? K<0, true> : K<0, false>))

extern "C" int ssdhip_sgd_step(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* bufs_h,
                               const long long* numel_h, int group, void* state, int rule, int nesterov, int tick, void* stream_) {
    if (rule < 0 || rule > 1) return SSDHIP_E_BADARG;
    return optim_state_step<SGD_CHUNK>(n_tensors, {params_h, grads_h, bufs_h}, numel_h, group, state, tick, stream_, sgd_tick_kernel,
                                       SGD_PICK(sgd_step_kernel, rule, nesterov));
}

extern "C" int ssdhip_sgd_step_bf16(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* master_h,
                                    void* const* bufs_h, const long long* numel_h, int group, void* state, int rule, int nesterov,
                                    int tick, void* stream_) {
    if (rule < 0 || rule > 1) return SSDHIP_E_BADARG;
    return optim_state_step<SGD_CHUNK>(n_tensors, {params_h, grads_h, master_h, bufs_h}, numel_h, group, state, tick, stream_,
                                       sgd_tick_kernel, SGD_PICK(sgd_step_bf16_kernel, rule, nesterov));
}

extern "C" int ssdhip_sgd_step_clipped(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* bufs_h,
                                       const long long* numel_h, int group, void* state, int rule, int nesterov, int tick, void* clip,
                                       void* stream_) {
    const ssdhip_clip_state* cl = optim_clip_block(clip);
    if (rule < 0 || rule > 1 || !cl) return SSDHIP_E_BADARG;
    return optim_state_step<SGD_CHUNK>(n_tensors, {params_h, grads_h, bufs_h}, numel_h, group, state, tick, stream_,
                                       sgd_tick_clipped_kernel, SGD_PICK(sgd_step_clipped_kernel, rule, nesterov), cl);
}

extern "C" int ssdhip_sgd_step_bf16_clipped(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* master_h,
                                            void* const* bufs_h, const long long* numel_h, int group, void* state, int rule, int nesterov,
                                            int tick, void* clip, void* stream_) {
    const ssdhip_clip_state* cl = optim_clip_block(clip);
    if (rule < 0 || rule > 1 || !cl) return SSDHIP_E_BADARG;
    return optim_state_step<SGD_CHUNK>(n_tensors, {params_h, grads_h, master_h, bufs_h}, numel_h, group, state, tick, stream_,
                                       sgd_tick_clipped_kernel, SGD_PICK(sgd_step_bf16_clipped_kernel, rule, nesterov), cl);
}
