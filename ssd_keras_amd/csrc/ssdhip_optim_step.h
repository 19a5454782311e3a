// ssdhip_optim_step.h -- what every optimizer step of libssdhip shares (ssdhip_optim.hip: SGD, ssdhip_adam.hip: Adam): the tensor table,
// ONE update body over it and ONE host launcher.  A step kernel names a rule (the per-element arithmetic, its scalars and how many
// float32 buffers a parameter has) and where its scalars come from; everything else -- which tensor a block works on, the vector
// passes, the scalar tail, the float32 and the bf16-with-master forms -- is optim_step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_bf16.h"

namespace ssdhip {

// Up to CHUNK tensors per launch, 4096 values per block.  The table travels in the KERNEL ARGUMENTS: gradients are new tensors every
// step (zero_grad(set_to_none=True)), and a device-side table would have to be re-uploaded -- a pageable host-to-device copy that
// blocks the host until the whole backward pass has drained (measured: the step 0.3-0.5 ms SLOWER than with the framework's optimizer
// although the kernels took 250 us less).  Columns, float32: p, g, buffers; bf16: p (written only), g, float32 master, buffers.
template <int NCOL, int CHUNK>
struct OptimTable {
    void* col[NCOL][CHUNK];
    long long n[CHUNK];
    int block0[CHUNK];                                     // first block of each tensor
    int count;
};

// The last tensor with block0 <= blk (uniform: scalar loads of the arguments).
template <class Table>
__device__ __forceinline__ int optim_tensor_of(const Table& a, int blk) {
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One block's 4096 values.  Rule::update(float& p, float g, float* bufs, const Scalars&) is one element of the update on p and its
// Rule::NBUF float32 buffers; with BF16 it runs on the float32 MASTER of a bf16 parameter: bf16 gradient in (exact in float32), weight
// decay on the master, p = bf16(master) out, round to nearest even, never read.  float32: four values per thread and pass (float4);
// bf16: eight (one 16-byte load of the gradients, two float4 each of master and buffers, one 16-byte store of the parameters).
// Every loop over the per-value arrays unrolls fully: they are registers.
template <class Rule, bool BF16, class Table>
__device__ __forceinline__ void optim_step(const Table& a, const typename Rule::Scalars& c) {
    constexpr int NB = Rule::NBUF, W = BF16 ? 8 : 4, BUF0 = BF16 ? 3 : 2;
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    const int k = optim_tensor_of(a, blk);
    bf16_t* p16 = static_cast<bf16_t*>(a.col[0][k]);
    const bf16_t* g16 = static_cast<const bf16_t*>(a.col[1][k]);
    const float* g32 = static_cast<const float*>(a.col[1][k]);
    float* w = static_cast<float*>(a.col[BF16 ? 2 : 0][k]);    // what the rule updates: the parameter, or its master
    float* buf[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) buf[b] = static_cast<float*>(a.col[BUF0 + b][k]);
    const long long n = a.n[k];
    const long long base = (long long)(blk - a.block0[k]) * 4096;
#pragma unroll
    for (int u = 0; u < 4096 / (256 * W); ++u) {
        const long long i = base + (long long)u * (256 * W) + tid * W;
        if (i + (W - 1) < n) {
            float ww[W], gg[W], bb[W][NB];
            if constexpr (BF16) {
                const uint4 gv = *reinterpret_cast<const uint4*>(g16 + i);
                const u32 gw[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                for (int q = 0; q < W; ++q) gg[q] = (q & 1) ? __uint_as_float(gw[q >> 1] & 0xffff0000u) : bf16_float(gw[q >> 1] & 0xffffu);
            } else {
                const float4 gv = *reinterpret_cast<const float4*>(g32 + i);
                gg[0] = gv.x, gg[1] = gv.y, gg[2] = gv.z, gg[3] = gv.w;
            }
#pragma unroll
            for (int h = 0; h < W / 4; ++h) {
                const float4 wv = *reinterpret_cast<const float4*>(w + i + 4 * h);
                ww[4 * h] = wv.x, ww[4 * h + 1] = wv.y, ww[4 * h + 2] = wv.z, ww[4 * h + 3] = wv.w;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float4 bv = *reinterpret_cast<const float4*>(buf[b] + i + 4 * h);
                    bb[4 * h][b] = bv.x, bb[4 * h + 1][b] = bv.y, bb[4 * h + 2][b] = bv.z, bb[4 * h + 3][b] = bv.w;
                }
            }
#pragma unroll
            for (int q = 0; q < W; ++q) Rule::update(ww[q], gg[q], bb[q], c);
#pragma unroll
            for (int h = 0; h < W / 4; ++h) {
                if (BF16) *reinterpret_cast<float4*>(w + i + 4 * h) = make_float4(ww[4 * h], ww[4 * h + 1], ww[4 * h + 2], ww[4 * h + 3]);
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    *reinterpret_cast<float4*>(buf[b] + i + 4 * h) = make_float4(bb[4 * h][b], bb[4 * h + 1][b], bb[4 * h + 2][b], bb[4 * h + 3][b]);
            }
            if constexpr (BF16)
                *reinterpret_cast<uint4*>(p16 + i) = make_uint4(pack2_bf16(ww[0], ww[1]), pack2_bf16(ww[2], ww[3]), pack2_bf16(ww[4], ww[5]),
                                                              pack2_bf16(ww[6], ww[7]));
            else
                *reinterpret_cast<float4*>(w + i) = make_float4(ww[0], ww[1], ww[2], ww[3]);
        } else {
            for (long long j = i; j < n && j < i + W; ++j) {
                float wq = w[j], bq[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) bq[b] = buf[b][j];
                Rule::update(wq, BF16 ? bf16_float(g16[j]) : g32[j], bq, c);
#pragma unroll
                for (int b = 0; b < NB; ++b) buf[b][j] = bq[b];
                w[j] = wq;
                if (BF16) p16[j] = bf16_bits<bf16_t>(wq);
            }
        }
    }
}

// A rule behind Keras's gradient clipping (Optimizer.get_gradients: clipnorm, then clipvalue, on the gradient of the penalised loss).
// The gradient is completed here -- t = g + wd * p, the value whose square ssdhip_grad_sumsq_partials summed --, scaled by what
// ssdhip_clip_finish left in the clip state block, clamped, and handed to Rule::update with the rule's own weight decay 0 so that the
// term is not applied twice.  One IEEE float32 operation each.  The multiplication always happens when clipnorm is on (scale is 1.0f
// when the norm is below it); the clamp is comparisons, so a NaN stays a NaN as in TensorFlow's minimum / maximum.  A step kernel
// names Clipped<Rule> where it named Rule: optim_step and the rules themselves do not know about clipping.
template <class Rule>
struct Clipped {
    static constexpr int NBUF = Rule::NBUF;
    struct Scalars {
        typename Rule::Scalars rule;                       // with weight decay 0
        float wd, scale, clipvalue;
        bool by_norm;
        __device__ Scalars(const typename Rule::Scalars& r, float wd_, const ssdhip_clip_state* __restrict__ cl)
            : rule(r), wd(wd_), scale(cl->scale), clipvalue(cl->clipvalue), by_norm(cl->clipnorm > 0.f) {}
    };
    static __device__ __forceinline__ void update(float& p, float g, float* bufs, const Scalars& c) {
        if (c.wd != 0.f) g = g + c.wd * p;
        if (c.by_norm) g = g * c.scale;
        if (c.clipvalue > 0.f) {
            g = g > c.clipvalue ? c.clipvalue : g;
            g = g < -c.clipvalue ? -c.clipvalue : g;
        }
        Rule::update(p, g, bufs, c.rule);
    }
};

// A group's base learning rate into a state block of either optimizer, stream-ordered.
template <class State>
__global__ __launch_bounds__(64) void optim_set_lr_kernel(State* st, int group, double lr) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && group < st->n_groups) st->groups[group].lr = lr;
}

template <class State>
int optim_set_lr(void* state, int group, double lr, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || group < 0 || group >= SSDHIP_ADAM_MAX_GROUPS || !(lr >= 0.0)) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(optim_set_lr_kernel<State>, dim3(1), dim3(64), 0, stream, static_cast<State*>(state), group, lr);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// The host side of every step: `cols` are the host arrays of device pointers in table order, `tick()` launches the optimizer's tick
// kernel if the call asks for it (false: the launch failed), `kernel(table, args...)` is the update.  EVERY check comes before the
// first launch -- nothing runs on a refused call, neither the tick nor an earlier chunk: pointers non-null and 16-byte aligned, sizes
// positive, a tensor's blocks and the grid of every launch (CHUNK tensors) within what `block0` and the grid can hold.
template <int CHUNK, int NCOL, class Tick, class Kernel, class... Args>
int optim_launch(hipStream_t stream, int n_tensors, const void* const* const (&cols)[NCOL], const long long* numel_h, Tick tick,
                 Kernel kernel, Args... args) {
    if (n_tensors <= 0 || !numel_h) return SSDHIP_E_BADARG;
    for (int c = 0; c < NCOL; ++c)
        if (!cols[c]) return SSDHIP_E_BADARG;
    long long chunk_blocks = 0;
    for (int k = 0; k < n_tensors; ++k) {
        uintptr_t bits = 0;
        for (int c = 0; c < NCOL; ++c) {
            if (!cols[c][k]) return SSDHIP_E_BADARG;
            bits |= (uintptr_t)cols[c][k];
        }
        if ((bits & 15) || numel_h[k] <= 0 || numel_h[k] > 0x3fffffffLL * 4096) return SSDHIP_E_BADARG;
        if (k % CHUNK == 0) chunk_blocks = 0;
        chunk_blocks += (numel_h[k] + 4095) / 4096;
        if (chunk_blocks > 0x7fffffffLL) return SSDHIP_E_BADARG;
    }
    if (!tick()) return SSDHIP_E_LAUNCH;
    for (int k0 = 0; k0 < n_tensors; k0 += CHUNK) {
        OptimTable<NCOL, CHUNK> a;
        a.count = n_tensors - k0 < CHUNK ? n_tensors - k0 : CHUNK;
        long long blocks = 0;
        for (int k = 0; k < CHUNK; ++k) {
            const int src = k < a.count ? k0 + k : k0;     // (unused slots repeat the first tensor: never selected)
            for (int c = 0; c < NCOL; ++c) a.col[c][k] = const_cast<void*>(cols[c][src]);
            a.n[k] = numel_h[src];
            a.block0[k] = (int)blocks;
            if (k < a.count) blocks += (numel_h[src] + 4095) / 4096;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a, args...);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }
    return SSDHIP_OK;
}

// The step of an optimizer whose scalars live in a state block: the block's own checks, then optim_launch behind the optimizer's tick.
// `extra`: what tick and update take behind their own arguments -- nothing, or the clip state block that ssdhip_clip_finish wrote for
// this step (the tick reads its skip decision, the update its scale).
template <int CHUNK, int NCOL, class State, class Kernel, class... Extra>
int optim_state_step(int n_tensors, const void* const* const (&cols)[NCOL], const long long* numel_h, int group, void* state, int tick,
                     void* stream_, void (*tick_kernel)(State*, Extra...), Kernel kernel, Extra... extra) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || group < 0 || group >= SSDHIP_ADAM_MAX_GROUPS) return SSDHIP_E_BADARG;
    State* st = static_cast<State*>(state);
    const auto ticker = [=] {
        if (tick) hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(SSDHIP_ADAM_MAX_GROUPS), 0, stream, st, extra...);
        return !tick || hipGetLastError() == hipSuccess;
    };
    return optim_launch<CHUNK>(stream, n_tensors, cols, numel_h, ticker, kernel, static_cast<const State*>(st), group, extra...);
}

// A clipped step's `clip` argument as the kernels take it; NULL where the call is to be refused (no block, or not 16-byte aligned).
inline const ssdhip_clip_state* optim_clip_block(const void* clip) {
    return ((uintptr_t)clip & 15) ? nullptr : static_cast<const ssdhip_clip_state*>(clip);
}

}  // namespace ssdhip
