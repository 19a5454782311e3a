// ssdhip_adam.hip -- keras.optimizers.Adam (Keras 2.x get_updates), the optimizer of every notebook of the reference but one
// (ssd7_training.ipynb:153, weight_sampling_tutorial.ipynb:533, the commented alternative of ssd300_training.ipynb:168), as ONE update
// launch over every parameter whose scalars live on the DEVICE.
//
// Adam's bias correction changes every step, so a captured step cannot carry it in its kernel arguments (sgd_momentum_kernel's `lr`
// replays with the value of the capture).  A small state block in global memory holds the step count, the running products beta^t and
// per parameter group the float32 scalars the update reads; a one-workgroup tick kernel advances it in front of the update.
//
//   adam_tick_kernel    iterations += 1; per group b1^t *= beta_1, b2^t *= beta_2 (running products in float64: the sequence NumPy
//                       reproduces to the bit, which pow() would not promise), Keras's time-based decay, and
//                       lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t) in float64, rounded once to float32.
//   AdamRule<AMSGRAD>   g += wd p (wd != 0); m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) (g g); [vh = max(vh, v)];
//                       p -= lr_t m / (sqrt(v) + eps) -- one IEEE float32 operation each, in this order (the build's -ffp-contract=off,
//                       hipcc's correctly rounded float32 divide and square root).
//   adam_step_kernel / adam_step_bf16_kernel
//                       that rule in the ONE update body every optimizer kernel shares (optim_step, ssdhip_optim_step.h: the tensor
//                       table in the kernel arguments, 4096 values per block, vector passes with a scalar tail), on float32 parameters
//                       and on the float32 MASTER copies of bf16 parameters.  28 bytes per parameter in both (4 x 4 + 3 x 4;
//                       2 + 8 + 8 + 8 + 2), 36 with amsgrad: pure streaming kernels.
//   adam_init_kernel    one thread: a group's hyperparameters (the products by `iterations` multiplications, so a restored optimizer
//                       continues the same float64 sequence).  The base learning rate: optim_set_lr_kernel, ssdhip_optim_step.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_bf16.h"
#include "ssdhip_optim_step.h"

namespace ssdhip {

__global__ __launch_bounds__(64) void adam_init_kernel(ssdhip_adam_state* st, int n_groups, int group, double lr, double beta_1,
                                                       double beta_2, double epsilon, double decay, double weight_decay,
                                                       long long iterations) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->iterations = iterations;
    st->n_groups = n_groups;
    st->reserved = 0;
    ssdhip_adam_group& s = st->groups[group];
    double b1t = 1.0, b2t = 1.0;
    // (linear in the restored step count, once per group and block: ~10 ns a step on one lane, a millisecond for the notebooks' 10^5
    //  steps; every group's call rewrites the same `iterations`)
    for (long long k = 0; k < iterations; ++k) {           // the tick's own sequence of products, not pow()
        b1t = b1t * beta_1;
        b2t = b2t * beta_2;
    }
    s.lr = lr;
    s.decay = decay;
    s.beta_1 = beta_1;
    s.beta_2 = beta_2;
    s.b1t = b1t;
    s.b2t = b2t;
    s.lr_t = 0.f;                                          // (the tick in front of every update writes it)
    s.one_minus_beta_1 = (float)(1.0 - beta_1);
    s.one_minus_beta_2 = (float)(1.0 - beta_2);
    s.beta_1_f = (float)beta_1;
    s.beta_2_f = (float)beta_2;
    s.epsilon = (float)epsilon;
    s.weight_decay = (float)weight_decay;
    s.reserved = 0;
}

// One workgroup, one thread per parameter group.
__device__ __forceinline__ void adam_tick(ssdhip_adam_state* st) {
    const int g = threadIdx.x;
    const long long t = st->iterations + 1;
    const int n_groups = st->n_groups;
    __syncthreads();                                       // every thread has read the old count
    if (g == 0) st->iterations = t;
    if (g >= n_groups) return;
    ssdhip_adam_group& s = st->groups[g];
    const double b1t = s.b1t * s.beta_1, b2t = s.b2t * s.beta_2;
    double lr = s.lr;
    if (s.decay > 0.0) lr = lr / (1.0 + s.decay * (double)(t - 1));   // Keras reads `iterations` before it increments it
    const double lr_t = lr * sqrt(1.0 - b2t) / (1.0 - b1t);
    s.b1t = b1t;
    s.b2t = b2t;
    s.lr_t = (float)lr_t;
}

__global__ __launch_bounds__(SSDHIP_ADAM_MAX_GROUPS) void adam_tick_kernel(ssdhip_adam_state* st) { adam_tick(st); }

// The tick of a clipped step: a skipped step (ssdhip_clip_finish's decision) leaves the count and the products as they are.
__global__ __launch_bounds__(SSDHIP_ADAM_MAX_GROUPS) void adam_tick_clipped_kernel(ssdhip_adam_state* st, const ssdhip_clip_state* clip) {
    if (clip->skip) return;
    adam_tick(st);
}

// One element of the update on p (the parameter, or its master) and its buffers m, v and, with amsgrad, vhat: one IEEE float32 operation
// per line part, in the order of include/ssdhip.h.
template <bool AMSGRAD>
struct AdamRule {
    static constexpr int NBUF = AMSGRAD ? 3 : 2;
    struct Scalars { float lr_t, omb1, omb2, b1, b2, eps, wd; };   // a group's, as the update reads them
    static __device__ __forceinline__ void update(float& p, float g, float* b, const Scalars& c) {
        float &m = b[0], &v = b[1], &vh = b[NBUF - 1];
        if (c.wd != 0.f) g = g + c.wd * p;
        m = c.b1 * m + c.omb1 * g;
        v = c.b2 * v + c.omb2 * (g * g);
        float den = v;
        if (AMSGRAD) {
            vh = vh >= v ? vh : v;
            den = vh;
        }
        p = p - c.lr_t * m / (__builtin_sqrtf(den) + c.eps);
    }
};

// Tensors per launch.  float32: p, g, m, v (+ vhat) = at most five pointers + count + first block = 52 bytes per tensor, 72 tensors are
// 3744 bytes of the 4 KB a launch may carry; bf16: the master as well, 60 bytes per tensor, 64 tensors are 3844 bytes.
constexpr int ADAM_CHUNK = 72, ADAM_BF16_CHUNK = 64;
template <bool AMSGRAD> using AdamArgs = OptimTable<2 + AdamRule<AMSGRAD>::NBUF, ADAM_CHUNK>;
template <bool AMSGRAD> using AdamBf16Args = OptimTable<3 + AdamRule<AMSGRAD>::NBUF, ADAM_BF16_CHUNK>;
static_assert(sizeof(AdamArgs<true>) + sizeof(void*) + sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");
static_assert(sizeof(AdamBf16Args<true>) + sizeof(void*) + sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");

// The group's scalars are the values the tick has just written (uniform: scalar loads).
template <bool AMSGRAD, bool BF16, class Table>
__device__ __forceinline__ void adam_step(const Table& a, const ssdhip_adam_state* __restrict__ st, int group) {
    if (group >= st->n_groups) return;
    const ssdhip_adam_group& s = st->groups[group];
    optim_step<AdamRule<AMSGRAD>, BF16>(a, {s.lr_t, s.one_minus_beta_1, s.one_minus_beta_2, s.beta_1_f, s.beta_2_f, s.epsilon, s.weight_decay});
}

template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_step_kernel(const AdamArgs<AMSGRAD> a, const ssdhip_adam_state* __restrict__ st, int group) {
    adam_step<AMSGRAD, false>(a, st, group);
}

template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_step_bf16_kernel(const AdamBf16Args<AMSGRAD> a, const ssdhip_adam_state* __restrict__ st,
                                                             int group) {
    adam_step<AMSGRAD, true>(a, st, group);
}

// The clipped forms: the same two kernels with Clipped<AdamRule> as their rule, nothing at all on a skipped step.
static_assert(sizeof(AdamArgs<true>) + 2 * sizeof(void*) + sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");
static_assert(sizeof(AdamBf16Args<true>) + 2 * sizeof(void*) + sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");

template <bool AMSGRAD, bool BF16, class Table>
__device__ __forceinline__ void adam_step_clipped(const Table& a, const ssdhip_adam_state* __restrict__ st, int group,
                                                  const ssdhip_clip_state* __restrict__ clip) {
    if (group >= st->n_groups || clip->skip) return;
    const ssdhip_adam_group& s = st->groups[group];
    optim_step<Clipped<AdamRule<AMSGRAD>>, BF16>(
        a, {{s.lr_t, s.one_minus_beta_1, s.one_minus_beta_2, s.beta_1_f, s.beta_2_f, s.epsilon, 0.f}, s.weight_decay, clip});
}

template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_step_clipped_kernel(const AdamArgs<AMSGRAD> a, const ssdhip_adam_state* __restrict__ st,
                                                                int group, const ssdhip_clip_state* __restrict__ clip) {
    adam_step_clipped<AMSGRAD, false>(a, st, group, clip);
}

template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_step_bf16_clipped_kernel(const AdamBf16Args<AMSGRAD> a, const ssdhip_adam_state* __restrict__ st,
                                                                     int group, const ssdhip_clip_state* __restrict__ clip) {
    adam_step_clipped<AMSGRAD, true>(a, st, group, clip);
}

}  // namespace ssdhip

using namespace ssdhip;

extern "C" size_t ssdhip_adam_state_bytes(int n_groups) {
    if (n_groups <= 0 || n_groups > SSDHIP_ADAM_MAX_GROUPS) return 0;
    return sizeof(ssdhip_adam_state) + (size_t)n_groups * sizeof(ssdhip_adam_group);
}

extern "C" int ssdhip_adam_state_init(void* state, int n_groups, int group, double lr, double beta_1, double beta_2, double epsilon,
                                      double decay, double weight_decay, long long iterations, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || n_groups <= 0 || n_groups > SSDHIP_ADAM_MAX_GROUPS || group < 0 || group >= n_groups)
        return SSDHIP_E_BADARG;
    if (!(lr >= 0.0) || !(beta_1 >= 0.0 && beta_1 < 1.0) || !(beta_2 >= 0.0 && beta_2 < 1.0) || !(epsilon >= 0.0) || !(decay >= 0.0)
        || !(weight_decay >= 0.0) || iterations < 0)
        return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(adam_init_kernel, dim3(1), dim3(64), 0, stream, static_cast<ssdhip_adam_state*>(state), n_groups, group, lr,
                       beta_1, beta_2, epsilon, decay, weight_decay, iterations);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_optim_set_lr(void* state, int group, double lr, void* stream_) {
    return optim_set_lr<ssdhip_adam_state>(state, group, lr, stream_);
}

// `vhat_h` is absent (no amsgrad) or one more column, non-null in every row like the others.
extern "C" int ssdhip_adam_step(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* m_h, void* const* v_h,
                                void* const* vhat_h, const long long* numel_h, int group, void* state, int tick, void* stream_) {
    if (vhat_h)
        return optim_state_step<ADAM_CHUNK>(n_tensors, {params_h, grads_h, m_h, v_h, vhat_h}, numel_h, group, state, tick, stream_,
                                            adam_tick_kernel, adam_step_kernel<true>);
    return optim_state_step<ADAM_CHUNK>(n_tensors, {params_h, grads_h, m_h, v_h}, numel_h, group, state, tick, stream_, adam_tick_kernel,
                                        adam_step_kernel<false>);
}

extern "C" int ssdhip_adam_step_bf16(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* master_h,
                                     void* const* m_h, void* const* v_h, void* const* vhat_h, const long long* numel_h, int group,
                                     void* state, int tick, void* stream_) {
    if (vhat_h)
        return optim_state_step<ADAM_BF16_CHUNK>(n_tensors, {params_h, grads_h, master_h, m_h, v_h, vhat_h}, numel_h, group, state, tick,
                                                 stream_, adam_tick_kernel, adam_step_bf16_kernel<true>);
    return optim_state_step<ADAM_BF16_CHUNK>(n_tensors, {params_h, grads_h, master_h, m_h, v_h}, numel_h, group, state, tick, stream_,
                                             adam_tick_kernel, adam_step_bf16_kernel<false>);
}

extern "C" int ssdhip_adam_step_clipped(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* m_h,
                                        void* const* v_h, void* const* vhat_h, const long long* numel_h, int group, void* state, int tick,
                                        void* clip, void* stream_) {
    const ssdhip_clip_state* cl = optim_clip_block(clip);
    if (!cl) return SSDHIP_E_BADARG;
    if (vhat_h)
        return optim_state_step<ADAM_CHUNK>(n_tensors, {params_h, grads_h, m_h, v_h, vhat_h}, numel_h, group, state, tick, stream_,
                                            adam_tick_clipped_kernel, adam_step_clipped_kernel<true>, cl);
    return optim_state_step<ADAM_CHUNK>(n_tensors, {params_h, grads_h, m_h, v_h}, numel_h, group, state, tick, stream_,
                                        adam_tick_clipped_kernel, adam_step_clipped_kernel<false>, cl);
}

extern "C" int ssdhip_adam_step_bf16_clipped(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* master_h,
                                             void* const* m_h, void* const* v_h, void* const* vhat_h, const long long* numel_h, int group,
                                             void* state, int tick, void* clip, void* stream_) {
    const ssdhip_clip_state* cl = optim_clip_block(clip);
    if (!cl) return SSDHIP_E_BADARG;
    if (vhat_h)
        return optim_state_step<ADAM_BF16_CHUNK>(n_tensors, {params_h, grads_h, master_h, m_h, v_h, vhat_h}, numel_h, group, state, tick,
                                                 stream_, adam_tick_clipped_kernel, adam_step_bf16_clipped_kernel<true>, cl);
    return optim_state_step<ADAM_BF16_CHUNK>(n_tensors, {params_h, grads_h, master_h, m_h, v_h}, numel_h, group, state, tick, stream_,
                                             adam_tick_clipped_kernel, adam_step_bf16_clipped_kernel<false>, cl);
}
