// ssdhip_fit.hip -- what a training LOOP needs from the device when its step is a replayed HIP graph (ssd_keras_amd/training.py,
// fit_generator): the value Keras reports as `loss` -- mean(compute_loss) + l2 * sum over the conv kernels of sum(w^2) -- accumulated
// over an epoch without the host reading anything per step, and the first non-finite batch loss latched for TerminateOnNaN.
//
//   sumsq_kernel<BF16>      one launch over a table of dense tensors (pointers and counts in the KERNEL ARGUMENTS, as SgdArgs of
//                           ssdhip_optim.hip: no device table, no upload).  The table's elements are cut into chunks of
//                           SSDHIP_SUMSQ_CHUNK = 8192, a tensor's last chunk short; one workgroup of 256 lanes per chunk, one float32
//                           partial per chunk, written exactly once by plain store.  No atomics, no last-workgroup finish, nothing to
//                           zero: the partials are summed by the meter's launch.
//                           The ORDER OF ADDITIONS is a function of the element index alone.  With V = 4 (float32) or 8 (bf16) values
//                           per 16-byte vector, element e of a chunk belongs to lane (e / V) % 256 and is that lane's value number
//                           (e / (256 V)) V + e % V; values past the tensor's end count as +0.
//                             per lane:      acc = 0;  acc = acc + x * x  over its 32 values in that order (float32, two roundings each)
//                             across lanes:  for s = 32, 16, 8, 4, 2, 1:  v[l] = v[l] + v[l + s]  (l < s), per wave of 64
//                             across waves:  ((w0 + w1) + w2) + w3
//                           The loads are 16 bytes per lane where the tensor's address allows it and 8, 4 or 2 bytes per load where
//                           it is only that much aligned (a slice of a larger buffer): the same values reach the same lanes, so the
//                           result does not depend on the alignment.  A tensor's tail is read element by element under its bound.
//   fit_meter_reset_kernel  writes every byte of a state block (a kernel, not a memset node: DESIGN.md 4.4).
//   fit_meter_update_kernel one workgroup: m = float32(sum_i float64(loss[i]) / B), q = float32(sum_j float64(partial[j])), both sums
//                           in index order by ONE lane (the others stage the values through LDS), batch_loss = m + l2 * q as two
//                           float32 operations; then the state: sum += float64(batch_loss) * B, seen += B, steps += 1, last, and
//                           first_bad = the step's index when batch_loss is not finite and nothing is latched yet.
//
// And what an optimizer that clips its gradients (Keras's clipnorm / clipvalue; ssd_keras_amd/optimizers.py) needs in front of its update:
//   grad_sumsq_kernel<BF16> sumsq_kernel's chunks and order of additions over x = g + wd * w, the gradient of the penalised loss, from a
//                           table of (gradient, float32 weight or none) pairs in the kernel arguments.
//   clip_init_kernel        writes every byte of a clip state block.
//   clip_finish_kernel      one workgroup: q = the partials summed in float64 in index order (serial_sum_f64, as the meter),
//                           norm = float32(sqrt(q)), scale = clipnorm / norm when norm >= clipnorm else 1, the skip decision of
//                           skip_nonfinite, the counters.  The clipped step kernels (ssdhip_optim_step.h) read the block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_math.h"
#include "ssdhip_bf16.h"

namespace ssdhip {

constexpr int SQ_WG = 256;                                 // lanes per workgroup
constexpr int SQ_PER_LANE = SSDHIP_SUMSQ_CHUNK / SQ_WG;    // 32 values per lane
constexpr int SQ_TENSORS = 128;                            // tensors per launch: 8 + 8 + 4 bytes each
struct SumsqArgs {
    const void* p[SQ_TENSORS];
    long long n[SQ_TENSORS];
    int block0[SQ_TENSORS];                                // first chunk of each tensor within this launch
    int count;
};
static_assert(sizeof(SumsqArgs) + sizeof(void*) + 8 <= 4096, "the tensor table must fit the kernel arguments");
static_assert(SSDHIP_SUMSQ_CHUNK % (SQ_WG * 8) == 0, "a chunk is whole passes of 16-byte vectors");

// V consecutive values starting at element e (e % V == 0, e + V <= n) of a tensor whose address is aligned to `al` bytes (a power of
// two, uniform over the workgroup): the widest loads `al` allows.
__device__ __forceinline__ void load_f32x4(const float* p, long long e, unsigned al, float* x) {
    if (al >= 16) {
        const float4 v = *reinterpret_cast<const float4*>(p + e);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else if (al >= 8) {
        const float2 a = *reinterpret_cast<const float2*>(p + e), b = *reinterpret_cast<const float2*>(p + e + 2);
        x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = p[e + j];
    }
}

__device__ __forceinline__ void load_bf16x8(const bf16_t* p, long long e, unsigned al, float* x) {
    u32 w[4];
    if (al >= 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(p + e);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else if (al >= 8) {
        const uint2 a = *reinterpret_cast<const uint2*>(p + e), b = *reinterpret_cast<const uint2*>(p + e + 4);
        w[0] = a.x, w[1] = a.y, w[2] = b.x, w[3] = b.y;
    } else if (al >= 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const u32*>(p + e + 2 * j);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (u32)p[e + 2 * j] | ((u32)p[e + 2 * j + 1] << 16);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[2 * j] = bf16_float(w[j] & 0xffffu);
        x[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
    }
}

// The last tensor of a table with block0 <= blk (uniform: scalar loads of the arguments).
template <class Args>
__device__ __forceinline__ int sumsq_tensor_of(const Args& a, int blk) {
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.block0[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// A chunk's values, U passes of V per lane, to its partial in the order of additions above: per lane, across the lanes of a wave,
// across the four waves.  Thread 0 stores.
template <int U, int V>
__device__ __forceinline__ void sumsq_chunk_store(const float (&x)[U][V], float* wave_sum, float* __restrict__ partial) {
    const int tid = threadIdx.x;
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < V; ++j) acc = acc + x[u][j] * x[u][j];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc = acc + __shfl_down(acc, s, 64);   // lane l < s: v[l] + v[l + s]; lane 0 holds the wave's sum
    if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) *partial = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

template <bool BF16>
__global__ __launch_bounds__(SQ_WG) void sumsq_kernel(const SumsqArgs a, float* __restrict__ partials, long long partial0) {
    constexpr int V = BF16 ? 8 : 4;                        // values per 16-byte vector
    constexpr int U = SQ_PER_LANE / V;                     // passes over the chunk
    __shared__ float wave_sum[SQ_WG / 64];
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    const int lo = sumsq_tensor_of(a, blk);
    const long long n = a.n[lo];
    const long long base = (long long)(blk - a.block0[lo]) * SSDHIP_SUMSQ_CHUNK;
    const uintptr_t addr = (uintptr_t)a.p[lo];
    const unsigned al = (addr & 15) == 0 ? 16u : (addr & 7) == 0 ? 8u : (addr & 3) == 0 ? 4u : 2u;
    float x[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {                          // every load of the chunk is in flight before the first addition
        const long long e = base + (long long)(u * SQ_WG + tid) * V;
        if (e + V <= n) {
            if (BF16) load_bf16x8(static_cast<const bf16_t*>(a.p[lo]), e, al, x[u]);
            else load_f32x4(static_cast<const float*>(a.p[lo]), e, al, x[u]);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float v = 0.f;
                if (e + j < n) v = BF16 ? bf16_float(static_cast<const bf16_t*>(a.p[lo])[e + j]) : static_cast<const float*>(a.p[lo])[e + j];
                x[u][j] = v;
            }
        }
    }
    sumsq_chunk_store(x, wave_sum, partials + partial0 + blk);
}

// The same partials with x = g + wd * w: the gradient of the penalised loss, the value an optimizer step forms first (g float32 or
// bf16, widened exactly; w the float32 parameter or master, or absent; wd == 0 reads no weight).  Two float32 operations, no fma.
constexpr int GQ_TENSORS = 128;                            // tensors per launch: 8 + 8 + 8 + 4 bytes each
struct GradSumsqArgs {
    const void* g[GQ_TENSORS];
    const float* w[GQ_TENSORS];
    long long n[GQ_TENSORS];
    int block0[GQ_TENSORS];
    int count;
};
static_assert(sizeof(GradSumsqArgs) + sizeof(void*) + 8 + 8 <= 4096, "the tensor table must fit the kernel arguments");

__device__ __forceinline__ unsigned align_of(const void* p) {
    const uintptr_t addr = (uintptr_t)p;
    return (addr & 15) == 0 ? 16u : (addr & 7) == 0 ? 8u : (addr & 3) == 0 ? 4u : 2u;
}

template <bool BF16>
__global__ __launch_bounds__(SQ_WG) void grad_sumsq_kernel(const GradSumsqArgs a, float wd, float* __restrict__ partials,
                                                           long long partial0) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr int U = SQ_PER_LANE / V;
    __shared__ float wave_sum[SQ_WG / 64];
    const int tid = threadIdx.x, blk = (int)blockIdx.x;
    const int lo = sumsq_tensor_of(a, blk);
    const long long n = a.n[lo];
    const long long base = (long long)(blk - a.block0[lo]) * SSDHIP_SUMSQ_CHUNK;
    const bf16_t* g16 = static_cast<const bf16_t*>(a.g[lo]);
    const float* g32 = static_cast<const float*>(a.g[lo]);
    const float* w = wd != 0.f ? a.w[lo] : nullptr;        // (uniform over the workgroup)
    const unsigned al_g = align_of(a.g[lo]), al_w = align_of(w);
    float x[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long e = base + (long long)(u * SQ_WG + tid) * V;
        if (e + V <= n) {
            if (BF16) load_bf16x8(g16, e, al_g, x[u]);
            else load_f32x4(g32, e, al_g, x[u]);
            if (w) {
                float ww[V];
#pragma unroll
                for (int h = 0; h < V / 4; ++h) load_f32x4(w, e + 4 * h, al_w, ww + 4 * h);
#pragma unroll
                for (int j = 0; j < V; ++j) x[u][j] = x[u][j] + wd * ww[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float v = 0.f;
                if (e + j < n) {
                    v = BF16 ? bf16_float(g16[e + j]) : g32[e + j];
                    if (w) v = v + wd * w[e + j];
                }
                x[u][j] = v;
            }
        }
    }
    sumsq_chunk_store(x, wave_sum, partials + partial0 + blk);
}

__global__ __launch_bounds__(64) void fit_meter_reset_kernel(ssdhip_fit_meter_state* st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->sum = 0.0;
    st->seen = 0;
    st->steps = 0;
    st->first_bad = -1;
    st->last = 0.f;
    st->reserved[0] = st->reserved[1] = st->reserved[2] = 0;
}

constexpr int METER_WG = 256;
constexpr int METER_TILE = 1024;

// sum_i float64(src[i]) in index order: every lane stages, lane 0 adds.  The result is lane 0's.
__device__ __forceinline__ double serial_sum_f64(const float* __restrict__ src, long long n, float* tile) {
    double s = 0.0;
    for (long long i0 = 0; i0 < n; i0 += METER_TILE) {
        const int m = (int)(n - i0 < METER_TILE ? n - i0 : METER_TILE);
        for (int i = threadIdx.x; i < m; i += METER_WG) tile[i] = src[i0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) s = s + (double)tile[i];
        __syncthreads();
    }
    return s;
}

__global__ __launch_bounds__(METER_WG) void fit_meter_update_kernel(const float* __restrict__ loss, int B, const float* __restrict__ partials,
                                                                    long long n_partials, float l2, ssdhip_fit_meter_state* st) {
    __shared__ float tile[METER_TILE];
    const double ls = serial_sum_f64(loss, B, tile);
    const double qs = serial_sum_f64(partials, n_partials, tile);
    if (threadIdx.x != 0) return;
    const float m = (float)(ls / (double)B);
    const float q = (float)qs;
    const float pen = l2 * q;
    const float batch_loss = m + pen;
    const long long step = st->steps;
    st->sum = st->sum + (double)batch_loss * (double)B;
    st->seen = st->seen + B;
    st->steps = step + 1;
    st->last = batch_loss;
    if ((__float_as_uint(batch_loss) & 0x7f800000u) == 0x7f800000u && st->first_bad < 0) st->first_bad = step;
}

// Every byte of a clip state block: the settings (0 = off), a step that clips nothing, the counters at zero.
__global__ __launch_bounds__(64) void clip_init_kernel(ssdhip_clip_state* st, float clipnorm, float clipvalue, int skip_nonfinite) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->q = 0.0;
    st->steps = st->clipped = st->skipped = 0;
    st->clipnorm = clipnorm;
    st->clipvalue = clipvalue;
    st->norm = 0.f;
    st->scale = 1.f;
    st->skip_nonfinite = skip_nonfinite;
    st->skip = 0;
    st->reserved[0] = st->reserved[1] = 0;
}

// One workgroup: the partials to q, norm, scale and the step's skip decision, as include/ssdhip.h spells them out.
__global__ __launch_bounds__(METER_WG) void clip_finish_kernel(const float* __restrict__ partials, long long n_partials,
                                                               ssdhip_clip_state* st) {
    __shared__ float tile[METER_TILE];
    const double q = serial_sum_f64(partials, n_partials, tile);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(q);
    const float clipnorm = st->clipnorm;
    const bool clip = clipnorm > 0.f && norm >= clipnorm;  // (a NaN norm compares false: the gradients stay as they are)
    const float scale = clip ? clipnorm / norm : 1.f;      // (an infinite norm: 0)
    const bool finite = (__double_as_longlong(q) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
    const bool skip = st->skip_nonfinite != 0 && !finite;
    st->q = q;
    st->norm = norm;
    st->scale = scale;
    st->skip = skip ? 1 : 0;
    st->steps = st->steps + 1;
    if (skip) st->skipped = st->skipped + 1;
    else if (clip) st->clipped = st->clipped + 1;
}

}  // namespace ssdhip

using namespace ssdhip;

extern "C" int ssdhip_sumsq_partials(int n_tensors, const void* const* tensors_h, const long long* numel_h, int dtype, float* partials,
                                     long long n_partials, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_tensors < 0 || n_partials < 0 || (dtype != SSDHIP_SUMSQ_F32 && dtype != SSDHIP_SUMSQ_BF16)) return SSDHIP_E_BADARG;
    if (n_tensors > 0 && (!tensors_h || !numel_h)) return SSDHIP_E_BADARG;
    const uintptr_t elem_mask = dtype == SSDHIP_SUMSQ_BF16 ? 1 : 3;
    long long total = 0;
    for (int k = 0; k < n_tensors; ++k) {                  // everything is checked before the first launch
        if (numel_h[k] < 0 || (numel_h[k] > 0 && (!tensors_h[k] || ((uintptr_t)tensors_h[k] & elem_mask)))) return SSDHIP_E_BADARG;
        total += (numel_h[k] + SSDHIP_SUMSQ_CHUNK - 1) / SSDHIP_SUMSQ_CHUNK;
        if (total > 0x7fffffffLL) return SSDHIP_E_BADARG;
    }
    if (total != n_partials) return SSDHIP_E_BADARG;       // the caller's buffer holds exactly one float32 per chunk
    if (total == 0) return SSDHIP_OK;
    if (!partials || ((uintptr_t)partials & 3)) return SSDHIP_E_BADARG;
    long long partial0 = 0;
    int k = 0;
    while (k < n_tensors) {
        SumsqArgs a;
        a.count = 0;
        long long blocks = 0;
        for (; k < n_tensors && a.count < SQ_TENSORS; ++k) {
            if (numel_h[k] == 0) continue;
            a.p[a.count] = tensors_h[k];
            a.n[a.count] = numel_h[k];
            a.block0[a.count] = (int)blocks;
            blocks += (numel_h[k] + SSDHIP_SUMSQ_CHUNK - 1) / SSDHIP_SUMSQ_CHUNK;
            ++a.count;
        }
        if (a.count == 0) break;
        for (int j = a.count; j < SQ_TENSORS; ++j) {       // (unused slots repeat the first tensor: never selected)
            a.p[j] = a.p[0];
            a.n[j] = a.n[0];
            a.block0[j] = 0;
        }
        if (dtype == SSDHIP_SUMSQ_BF16)
            hipLaunchKernelGGL((sumsq_kernel<true>), dim3((unsigned)blocks), dim3(SQ_WG), 0, stream, a, partials, partial0);
        else
            hipLaunchKernelGGL((sumsq_kernel<false>), dim3((unsigned)blocks), dim3(SQ_WG), 0, stream, a, partials, partial0);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
        partial0 += blocks;
    }
    return SSDHIP_OK;
}

extern "C" int ssdhip_grad_sumsq_partials(int n_tensors, const void* const* grads_h, const void* const* weights_h,
                                          const long long* numel_h, int dtype, double weight_decay, float* partials, long long n_partials,
                                          void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_tensors < 0 || n_partials < 0 || (dtype != SSDHIP_SUMSQ_F32 && dtype != SSDHIP_SUMSQ_BF16)) return SSDHIP_E_BADARG;
    if (n_tensors > 0 && (!grads_h || !numel_h)) return SSDHIP_E_BADARG;
    const float wd = (float)weight_decay;
    if (!(weight_decay >= 0.0) || !(wd <= 3.402823466e38f)) return SSDHIP_E_BADARG;
    const uintptr_t elem_mask = dtype == SSDHIP_SUMSQ_BF16 ? 1 : 3;
    long long total = 0;
    for (int k = 0; k < n_tensors; ++k) {                  // everything is checked before the first launch
        if (numel_h[k] < 0 || (numel_h[k] > 0 && (!grads_h[k] || ((uintptr_t)grads_h[k] & elem_mask)))) return SSDHIP_E_BADARG;
        if (weights_h && ((uintptr_t)weights_h[k] & 3)) return SSDHIP_E_BADARG;
        total += (numel_h[k] + SSDHIP_SUMSQ_CHUNK - 1) / SSDHIP_SUMSQ_CHUNK;
        if (total > 0x7fffffffLL) return SSDHIP_E_BADARG;
    }
    if (total != n_partials) return SSDHIP_E_BADARG;       // the caller's buffer holds exactly one float32 per chunk
    if (total == 0) return SSDHIP_OK;
    if (!partials || ((uintptr_t)partials & 3)) return SSDHIP_E_BADARG;
    long long partial0 = 0;
    int k = 0;
    while (k < n_tensors) {
        GradSumsqArgs a;
        a.count = 0;
        long long blocks = 0;
        for (; k < n_tensors && a.count < GQ_TENSORS; ++k) {
            if (numel_h[k] == 0) continue;
            a.g[a.count] = grads_h[k];
            a.w[a.count] = weights_h ? static_cast<const float*>(weights_h[k]) : nullptr;
            a.n[a.count] = numel_h[k];
            a.block0[a.count] = (int)blocks;
            blocks += (numel_h[k] + SSDHIP_SUMSQ_CHUNK - 1) / SSDHIP_SUMSQ_CHUNK;
            ++a.count;
        }
        if (a.count == 0) break;
        for (int j = a.count; j < GQ_TENSORS; ++j) {       // (unused slots repeat the first tensor: never selected)
            a.g[j] = a.g[0];
            a.w[j] = a.w[0];
            a.n[j] = a.n[0];
            a.block0[j] = 0;
        }
        if (dtype == SSDHIP_SUMSQ_BF16)
            hipLaunchKernelGGL((grad_sumsq_kernel<true>), dim3((unsigned)blocks), dim3(SQ_WG), 0, stream, a, wd, partials, partial0);
        else
            hipLaunchKernelGGL((grad_sumsq_kernel<false>), dim3((unsigned)blocks), dim3(SQ_WG), 0, stream, a, wd, partials, partial0);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
        partial0 += blocks;
    }
    return SSDHIP_OK;
}

extern "C" size_t ssdhip_clip_state_bytes(void) { return sizeof(ssdhip_clip_state); }

extern "C" int ssdhip_clip_state_init(void* state, double clipnorm, double clipvalue, int skip_nonfinite, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || !(clipnorm >= 0.0) || !(clipvalue >= 0.0)) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(clip_init_kernel, dim3(1), dim3(64), 0, stream, static_cast<ssdhip_clip_state*>(state), (float)clipnorm,
                       (float)clipvalue, skip_nonfinite ? 1 : 0);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_clip_finish(const float* partials, long long n_partials, void* state, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || n_partials < 0) return SSDHIP_E_BADARG;
    if (n_partials > 0 && (!partials || ((uintptr_t)partials & 3))) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(METER_WG), 0, stream, partials, n_partials, static_cast<ssdhip_clip_state*>(state));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" size_t ssdhip_fit_meter_state_bytes(void) { return sizeof(ssdhip_fit_meter_state); }

extern "C" int ssdhip_fit_meter_reset(void* state, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15)) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(fit_meter_reset_kernel, dim3(1), dim3(64), 0, stream, static_cast<ssdhip_fit_meter_state*>(state));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_fit_meter_update(const float* loss, int B, const float* partials, long long n_partials, float l2, void* state,
                                       void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!state || ((uintptr_t)state & 15) || !loss || ((uintptr_t)loss & 3) || B <= 0 || n_partials < 0) return SSDHIP_E_BADARG;
    if (n_partials > 0 && (!partials || ((uintptr_t)partials & 3))) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(fit_meter_update_kernel, dim3(1), dim3(METER_WG), 0, stream, loss, B, partials, n_partials, l2,
                       static_cast<ssdhip_fit_meter_state*>(state));
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
