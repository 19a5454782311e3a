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
//   adam_step_kernel    g += wd p (wd != 0); m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) (g g); [vh = max(vh, v)];
//                       p -= lr_t m / (sqrt(v) + eps) -- one IEEE float32 operation each, in this order (the build's -ffp-contract=off,
//                       hipcc's correctly rounded float32 divide and square root).  Shaped like sgd_momentum_kernel: the tensor table in
//                       the kernel arguments, 4096 values per block, float4 accesses with a scalar tail.  28 bytes per parameter
//                       (36 with amsgrad): a pure streaming kernel.
//   adam_step_bf16_kernel   the same update (adam_update, shared with adam_step_kernel) on a float32 MASTER copy of a bf16 parameter: the
//                       gradient is bf16 (exact in float32), weight decay reads the master, and p = bf16(master), round to nearest
//                       even, is written without ever being read.  Eight values per thread and pass: one 16-byte load of the gradients,
//                       two float4 each of master and moments, one 16-byte store of the parameters.  28 bytes per parameter as well
//                       (2 + 8 + 8 + 8 + 2; 36 with amsgrad).
//   adam_init_kernel / optim_set_lr_kernel   one thread each: a group's hyperparameters (the products by `iterations` multiplications,
//                       so a restored optimizer continues the same float64 sequence) / a group's base learning rate, stream-ordered.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_bf16.h"

namespace ssdhip {

// Five pointers + count + first block = 52 bytes per tensor: 72 tensors are 3744 bytes of the 4 KB a launch may carry.
constexpr int ADAM_CHUNK = 72;
struct AdamArgs {
    float* p[ADAM_CHUNK];
    const float* g[ADAM_CHUNK];
    float* m[ADAM_CHUNK];
    float* v[ADAM_CHUNK];
    float* vh[ADAM_CHUNK];                                 // amsgrad only (else the slots repeat v: never read)
    long long n[ADAM_CHUNK];
    int block0[ADAM_CHUNK];                                // first block of each tensor (4096 values per block)
    int count;
};
static_assert(sizeof(AdamArgs) + sizeof(void*) + sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");

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

__global__ __launch_bounds__(64) void optim_set_lr_kernel(ssdhip_adam_state* st, int group, double lr) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && group < st->n_groups) st->groups[group].lr = lr;
}

// One workgroup, one thread per parameter group.
__global__ __launch_bounds__(SSDHIP_ADAM_MAX_GROUPS) void adam_tick_kernel(ssdhip_adam_state* st) {
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

// Six pointers + count + first block = 60 bytes per tensor: 64 tensors are 3844 bytes.
constexpr int ADAM_BF16_CHUNK = 64;
struct AdamBf16Args {
    bf16_t* p[ADAM_BF16_CHUNK];                            // written only
    const bf16_t* g[ADAM_BF16_CHUNK];
    float* w[ADAM_BF16_CHUNK];                             // the float32 master
    float* m[ADAM_BF16_CHUNK];
    float* v[ADAM_BF16_CHUNK];
    float* vh[ADAM_BF16_CHUNK];                            // amsgrad only (else the slots repeat v: never read)
    long long n[ADAM_BF16_CHUNK];
    int block0[ADAM_BF16_CHUNK];
    int count;
};
static_assert(sizeof(AdamBf16Args) + sizeof(void*) + sizeof(int) <= 4096, "the tensor table must fit the kernel arguments");

// The scalars of a group as the update reads them.
struct AdamScalars {
    float lr_t, omb1, omb2, b1, b2, eps, wd;
};
__device__ __forceinline__ AdamScalars adam_scalars(const ssdhip_adam_group& s) {
    return {s.lr_t, s.one_minus_beta_1, s.one_minus_beta_2, s.beta_1_f, s.beta_2_f, s.epsilon, s.weight_decay};
}

// One element of the update, for the float32 kernel (p is the parameter) and the bf16 one (p is its master): one IEEE float32 operation
// per line part, in the order of include/ssdhip.h.
template <bool AMSGRAD>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float& vh, const AdamScalars& c) {
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

template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_step_kernel(const AdamArgs a, const ssdhip_adam_state* __restrict__ st, int group) {
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    if (group >= st->n_groups) return;
    const AdamScalars c = adam_scalars(st->groups[group]);  // uniform: scalar loads, the values the tick has just written
    int lo = 0, hi = a.count - 1;                          // last tensor with block0 <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    float* p = a.p[lo];
    const float* g = a.g[lo];
    float* m = a.m[lo];
    float* v = a.v[lo];
    float* vh = a.vh[lo];
    const long long n = a.n[lo];
    const long long base = (long long)(blk - a.block0[lo]) * 4096;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long i = base + (long long)u * 1024 + tid * 4;
        if (i + 3 < n) {
            const float4 pv = *reinterpret_cast<const float4*>(p + i), gv = *reinterpret_cast<const float4*>(g + i);
            const float4 mv = *reinterpret_cast<const float4*>(m + i), vv = *reinterpret_cast<const float4*>(v + i);
            float4 hv = vv;
            if (AMSGRAD) hv = *reinterpret_cast<const float4*>(vh + i);
            float gg[4] = {gv.x, gv.y, gv.z, gv.w}, pp[4] = {pv.x, pv.y, pv.z, pv.w}, mm[4] = {mv.x, mv.y, mv.z, mv.w};
            float v2[4] = {vv.x, vv.y, vv.z, vv.w}, hh[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) adam_update<AMSGRAD>(pp[q], gg[q], mm[q], v2[q], hh[q], c);
            *reinterpret_cast<float4*>(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *reinterpret_cast<float4*>(v + i) = make_float4(v2[0], v2[1], v2[2], v2[3]);
            if (AMSGRAD) *reinterpret_cast<float4*>(vh + i) = make_float4(hh[0], hh[1], hh[2], hh[3]);
            *reinterpret_cast<float4*>(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
        } else {
            for (long long j = i; j < n && j < i + 4; ++j) {
                float pq = p[j], mq = m[j], vq = v[j], hq = AMSGRAD ? vh[j] : 0.f;
                adam_update<AMSGRAD>(pq, g[j], mq, vq, hq, c);
                if (AMSGRAD) vh[j] = hq;
                m[j] = mq;
                v[j] = vq;
                p[j] = pq;
            }
        }
    }
}

// The same launch shape over bf16 parameters with float32 masters: 4096 values per block, eight per thread and pass.
template <bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_step_bf16_kernel(const AdamBf16Args a, const ssdhip_adam_state* __restrict__ st, int group) {
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    if (group >= st->n_groups) return;
    const AdamScalars c = adam_scalars(st->groups[group]);
    int lo = 0, hi = a.count - 1;                          // last tensor with block0 <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    bf16_t* p = a.p[lo];
    const bf16_t* g = a.g[lo];
    float* w = a.w[lo];
    float* m = a.m[lo];
    float* v = a.v[lo];
    float* vh = a.vh[lo];
    const long long n = a.n[lo];
    const long long base = (long long)(blk - a.block0[lo]) * 4096;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long long i = base + (long long)u * 2048 + tid * 8;
        if (i + 7 < n) {
            const uint4 gv = *reinterpret_cast<const uint4*>(g + i);
            const u32 gw[4] = {gv.x, gv.y, gv.z, gv.w};
            float ww[8], mm[8], v2[8], hh[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 wv = *reinterpret_cast<const float4*>(w + i + 4 * h), mv = *reinterpret_cast<const float4*>(m + i + 4 * h);
                const float4 vv = *reinterpret_cast<const float4*>(v + i + 4 * h);
                float4 hv = vv;
                if (AMSGRAD) hv = *reinterpret_cast<const float4*>(vh + i + 4 * h);
                ww[4 * h] = wv.x, ww[4 * h + 1] = wv.y, ww[4 * h + 2] = wv.z, ww[4 * h + 3] = wv.w;
                mm[4 * h] = mv.x, mm[4 * h + 1] = mv.y, mm[4 * h + 2] = mv.z, mm[4 * h + 3] = mv.w;
                v2[4 * h] = vv.x, v2[4 * h + 1] = vv.y, v2[4 * h + 2] = vv.z, v2[4 * h + 3] = vv.w;
                hh[4 * h] = hv.x, hh[4 * h + 1] = hv.y, hh[4 * h + 2] = hv.z, hh[4 * h + 3] = hv.w;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float gq = (q & 1) ? __uint_as_float(gw[q >> 1] & 0xffff0000u) : bf16_float(gw[q >> 1] & 0xffffu);
                adam_update<AMSGRAD>(ww[q], gq, mm[q], v2[q], hh[q], c);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                *reinterpret_cast<float4*>(w + i + 4 * h) = make_float4(ww[4 * h], ww[4 * h + 1], ww[4 * h + 2], ww[4 * h + 3]);
                *reinterpret_cast<float4*>(m + i + 4 * h) = make_float4(mm[4 * h], mm[4 * h + 1], mm[4 * h + 2], mm[4 * h + 3]);
                *reinterpret_cast<float4*>(v + i + 4 * h) = make_float4(v2[4 * h], v2[4 * h + 1], v2[4 * h + 2], v2[4 * h + 3]);
                if (AMSGRAD) *reinterpret_cast<float4*>(vh + i + 4 * h) = make_float4(hh[4 * h], hh[4 * h + 1], hh[4 * h + 2], hh[4 * h + 3]);
            }
            *reinterpret_cast<uint4*>(p + i) = make_uint4(pack2_bf16(ww[0], ww[1]), pack2_bf16(ww[2], ww[3]), pack2_bf16(ww[4], ww[5]),
                                                          pack2_bf16(ww[6], ww[7]));
        } else {
            for (long long j = i; j < n && j < i + 8; ++j) {
                float wq = w[j], mq = m[j], vq = v[j], hq = AMSGRAD ? vh[j] : 0.f;
                adam_update<AMSGRAD>(wq, bf16_float(g[j]), mq, vq, hq, c);
                if (AMSGRAD) vh[j] = hq;
                m[j] = mq;
                v[j] = vq;
                w[j] = wq;
                p[j] = bf16_bits<bf16_t>(wq);
            }
        }
    }
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
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || group < 0 || group >= SSDHIP_ADAM_MAX_GROUPS || !(lr >= 0.0)) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(optim_set_lr_kernel, dim3(1), dim3(64), 0, stream, static_cast<ssdhip_adam_state*>(state), group, lr);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_adam_step(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* m_h, void* const* v_h,
                                void* const* vhat_h, const long long* numel_h, int group, void* state, int tick, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_tensors <= 0 || !params_h || !grads_h || !m_h || !v_h || !numel_h || !state || ((uintptr_t)state & 15) || group < 0
        || group >= SSDHIP_ADAM_MAX_GROUPS)
        return SSDHIP_E_BADARG;
    for (int k = 0; k < n_tensors; ++k) {
        if (!params_h[k] || !grads_h[k] || !m_h[k] || !v_h[k] || (vhat_h && !vhat_h[k]) || numel_h[k] <= 0) return SSDHIP_E_BADARG;
        if (((uintptr_t)params_h[k] | (uintptr_t)grads_h[k] | (uintptr_t)m_h[k] | (uintptr_t)v_h[k]
             | (vhat_h ? (uintptr_t)vhat_h[k] : 0)) & 15)
            return SSDHIP_E_BADARG;
        if ((numel_h[k] + 4095) / 4096 > 0x3fffffffLL) return SSDHIP_E_BADARG;
    }
    ssdhip_adam_state* st = static_cast<ssdhip_adam_state*>(state);
    if (tick) {
        hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(SSDHIP_ADAM_MAX_GROUPS), 0, stream, st);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    for (int k0 = 0; k0 < n_tensors; k0 += ADAM_CHUNK) {
        AdamArgs a;
        a.count = n_tensors - k0 < ADAM_CHUNK ? n_tensors - k0 : ADAM_CHUNK;
        long long blocks = 0;
        for (int k = 0; k < ADAM_CHUNK; ++k) {
            const int src = k < a.count ? k0 + k : k0;     // (unused slots repeat the first tensor: never selected)
            a.p[k] = static_cast<float*>(params_h[src]);
            a.g[k] = static_cast<const float*>(grads_h[src]);
            a.m[k] = static_cast<float*>(m_h[src]);
            a.v[k] = static_cast<float*>(v_h[src]);
            a.vh[k] = static_cast<float*>(vhat_h ? vhat_h[src] : v_h[src]);
            a.n[k] = numel_h[src];
            a.block0[k] = (int)blocks;
            if (k < a.count) blocks += (numel_h[src] + 4095) / 4096;
            if (blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
        }
        if (vhat_h)
            hipLaunchKernelGGL(adam_step_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a, st, group);
        else
            hipLaunchKernelGGL(adam_step_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a, st, group);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    return SSDHIP_OK;
}

extern "C" int ssdhip_adam_step_bf16(int n_tensors, void* const* params_h, const void* const* grads_h, void* const* master_h,
                                     void* const* m_h, void* const* v_h, void* const* vhat_h, const long long* numel_h, int group,
                                     void* state, int tick, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_tensors <= 0 || !params_h || !grads_h || !master_h || !m_h || !v_h || !numel_h || !state || ((uintptr_t)state & 15) || group < 0
        || group >= SSDHIP_ADAM_MAX_GROUPS)
        return SSDHIP_E_BADARG;
    long long chunk_blocks = 0;
    for (int k = 0; k < n_tensors; ++k) {
        if (!params_h[k] || !grads_h[k] || !master_h[k] || !m_h[k] || !v_h[k] || (vhat_h && !vhat_h[k]) || numel_h[k] <= 0)
            return SSDHIP_E_BADARG;
        if (((uintptr_t)params_h[k] | (uintptr_t)grads_h[k] | (uintptr_t)master_h[k] | (uintptr_t)m_h[k] | (uintptr_t)v_h[k]
             | (vhat_h ? (uintptr_t)vhat_h[k] : 0)) & 15)
            return SSDHIP_E_BADARG;
        if ((numel_h[k] + 4095) / 4096 > 0x3fffffffLL) return SSDHIP_E_BADARG;
        if (k % ADAM_BF16_CHUNK == 0) chunk_blocks = 0;     // (a launch's grid, before the tick: nothing runs on a refused call)
        chunk_blocks += (numel_h[k] + 4095) / 4096;
        if (chunk_blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
    }
    ssdhip_adam_state* st = static_cast<ssdhip_adam_state*>(state);
    if (tick) {
        hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(SSDHIP_ADAM_MAX_GROUPS), 0, stream, st);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    for (int k0 = 0; k0 < n_tensors; k0 += ADAM_BF16_CHUNK) {
        AdamBf16Args a;
        a.count = n_tensors - k0 < ADAM_BF16_CHUNK ? n_tensors - k0 : ADAM_BF16_CHUNK;
        long long blocks = 0;
        for (int k = 0; k < ADAM_BF16_CHUNK; ++k) {
            const int src = k < a.count ? k0 + k : k0;     // (unused slots repeat the first tensor: never selected)
            a.p[k] = static_cast<bf16_t*>(params_h[src]);
            a.g[k] = static_cast<const bf16_t*>(grads_h[src]);
            a.w[k] = static_cast<float*>(master_h[src]);
            a.m[k] = static_cast<float*>(m_h[src]);
            a.v[k] = static_cast<float*>(v_h[src]);
            a.vh[k] = static_cast<float*>(vhat_h ? vhat_h[src] : v_h[src]);
            a.n[k] = numel_h[src];
            a.block0[k] = (int)blocks;
            if (k < a.count) blocks += (numel_h[src] + 4095) / 4096;
        }
        if (vhat_h)
            hipLaunchKernelGGL(adam_step_bf16_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a, st, group);
        else
            hipLaunchKernelGGL(adam_step_bf16_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a, st, group);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    return SSDHIP_OK;
}
