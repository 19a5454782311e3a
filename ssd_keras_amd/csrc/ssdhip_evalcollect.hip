// ssdhip_evalcollect.hip -- Evaluator.predict_on_dataset's collection on gfx950 (MI355X): the stretch between the decoder's output
// and ssdhip_match_predictions_multi's input (eval_utils/average_precision_evaluator.py:395-424 and :629-634 of the reference).
//
// The host path downloads every batch of decoded rows, runs each image's inverse transforms as Python closures, rounds every box
// through NumPy scalars into per-class lists of tuples, and later walks those tuples again to build the matcher's arrays.  Here the
// rows never leave the device:
//   ssdhip_eval_collect   appends one batch's valid rows, inverted and rounded in the rows' own dtype, to a device-resident store in
//                         (image, row) order.  Two launches: evc_plan_kernel (ONE workgroup: per-image valid counts, their prefix, the
//                         capacity check, and the advance of the store's append counter -- the only writer of that counter, so there
//                         is no host read per batch and no race) and evc_collect_kernel (one workgroup per image: in-block ranks from
//                         ballots, so a row's position never depends on scheduling).
//   ssdhip_eval_pack      a stable counting sort of the store by class: evp_count_kernel (per-chunk per-class counts),
//                         evp_scan_kernel (ONE workgroup: exclusive prefix over (class, chunk)), evp_scatter_kernel (in-chunk ranks
//                         from ballots plus per-wave class counts).  Integer atomics only ever COUNT (LDS histograms, the store's
//                         statistics); no position is decided by one, there are no float atomics and no memset nodes.
// The arithmetic is the reference's, one IEEE rounding per operation (-ffp-contract=off): Resize's inverter v = rint(v * T(s)),
// CropPad's v = v + T(d), round(v, n) = rint(v * T(10^n)) / T(10^n), all in the rows' dtype T (tests/np_eval_collect.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"

namespace ssdhip {

typedef unsigned long long evc_u64;

constexpr int EVC_PLAN_THREADS = 1024;      // = the largest batch: one LDS slot per image
constexpr int EVC_THREADS = 256;
constexpr int EVC_WAVES = EVC_THREADS / 64;
constexpr int EVP_CHUNK = SSDHIP_EVAL_PACK_CHUNK;
constexpr int EVP_WAVES = EVP_CHUNK / 64;
constexpr int EVP_SCAN_THREADS = 1024;
constexpr int EVC_MAXC = SSDHIP_EVAL_MAX_CLASSES;

__device__ __forceinline__ float evc_rint(float v) { return rintf(v); }
__device__ __forceinline__ double evc_rint(double v) { return rint(v); }

// the class of a row as the host's `int(box[class_id])` files it: 1 .. n_classes, or 0 for everything results[class_id] has no list for
template <typename T>
__device__ __forceinline__ int evc_class(T v, int n_classes) {
    return (v >= (T)1 && v < (T)(n_classes + 1)) ? (int)v : 0;
}

// exclusive prefix of `v` over the workgroup (blockDim.x = 64 * n_waves), total in `total`; `wsum` holds n_waves ints
__device__ __forceinline__ int evc_block_exclusive(int v, int* wsum, int n_waves, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();                         // wsum may still be read from the previous use
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < n_waves; ++i) {
        const int s = wsum[i];
        if (i < w) before += s;
        all += s;
    }
    total = all;
    return before + inc - v;
}

// ---- collect -----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(EVC_PLAN_THREADS) void evc_plan_kernel(const T* __restrict__ rows, int B, int R, const int* __restrict__ count,
                                                                    int capacity, int* __restrict__ counters, int* __restrict__ plan) {
    __shared__ int cnt[EVC_PLAN_THREADS];
    __shared__ int wsum[EVC_PLAN_THREADS / 64];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int b = w; b < B; b += EVC_PLAN_THREADS / 64) {     // one wave per image
        int c = 0;
        if (count) {
            c = count[b];
            c = c < 0 ? 0 : (c > R ? R : c);
        } else {
            for (int r0 = 0; r0 < R; r0 += 64) {
                const int r = r0 + lane;
                const bool valid = r < R && rows[((size_t)b * R + r) * 6] != (T)0;
                c += __popcll(__ballot(valid));
            }
        }
        if (lane == 0) cnt[b] = c;
    }
    __syncthreads();
    const int mine = tid < B ? cnt[tid] : 0;
    int total;
    const int before = evc_block_exclusive(mine, wsum, EVC_PLAN_THREADS / 64, total);
    if (tid == 0) {
        const int base = counters[SSDHIP_EVAL_N_ROWS];
        const bool fits = base >= 0 && (long long)base + (long long)total <= (long long)capacity;
        if (fits) counters[SSDHIP_EVAL_N_ROWS] = base + total;
        else counters[SSDHIP_EVAL_OVERFLOW] = 1;
        base_s = fits ? base : -1;
    }
    __syncthreads();
    if (tid < B) {
        plan[tid] = base_s < 0 ? -1 : base_s + before;
        plan[B + tid] = mine;
    }
}

template <typename T>
__global__ __launch_bounds__(EVC_THREADS) void evc_collect_kernel(const T* __restrict__ rows, int B, int R, const int* __restrict__ count,
                                                                  const double* __restrict__ desc, int n_images, int n_classes,
                                                                  T coord_pow, T conf_pow, T* __restrict__ store_rows,
                                                                  int* __restrict__ store_image, int capacity, int* __restrict__ counters,
                                                                  const int* __restrict__ plan) {
    __shared__ int hist[EVC_MAXC + 1];
    __shared__ int wsum[EVC_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int start = plan[b], n = plan[B + b];
    if (start < 0 || n <= 0) return;                         // the append did not fit, or an image without rows: nothing to do
    for (int c = tid; c <= n_classes; c += EVC_THREADS) hist[c] = 0;
    const double* d = desc + (size_t)b * SSDHIP_EVAL_DESC;
    const int image = (d[0] >= 0.0 && d[0] < (double)n_images) ? (int)d[0] : -1;
    const int n_steps = (d[1] >= 0.0 && d[1] <= (double)SSDHIP_EVAL_MAX_STEPS) ? (int)d[1] : 0;
    int running = 0;
    for (int r0 = 0; r0 < R; r0 += EVC_THREADS) {
        const int r = r0 + tid;
        const T* src = rows + ((size_t)b * R + (r < R ? r : 0)) * 6;
        const T cls = src[0];
        const bool valid = r < R && (count ? r < n : cls != (T)0);
        int total;
        const int rank = running + evc_block_exclusive(valid ? 1 : 0, wsum, EVC_WAVES, total);
        running += total;
        if (!valid) continue;
        T conf = src[1], xmin = src[2], ymin = src[3], xmax = src[4], ymax = src[5];
        for (int k = 0; k < n_steps; ++k) {
            const T ay = (T)d[2 + 3 * k + 1], ax = (T)d[2 + 3 * k + 2];
            if (d[2 + 3 * k] == 0.0) {                       // scale: Resize's inverter
                ymin = evc_rint(ymin * ay); ymax = evc_rint(ymax * ay);
                xmin = evc_rint(xmin * ax); xmax = evc_rint(xmax * ax);
            } else {                                         // shift: CropPad's
                ymin = ymin + ay; ymax = ymax + ay;
                xmin = xmin + ax; xmax = xmax + ax;
            }
        }
        if (conf_pow != (T)0) conf = evc_rint(conf * conf_pow) / conf_pow;
        if (coord_pow != (T)0) {
            xmin = evc_rint(xmin * coord_pow) / coord_pow; ymin = evc_rint(ymin * coord_pow) / coord_pow;
            xmax = evc_rint(xmax * coord_pow) / coord_pow; ymax = evc_rint(ymax * coord_pow) / coord_pow;
        }
        const int dst = start + rank;
        if (rank < n && dst < capacity) {                    // the plan promises both
            T* out = store_rows + (size_t)dst * 6;
            out[0] = cls; out[1] = conf; out[2] = xmin; out[3] = ymin; out[4] = xmax; out[5] = ymax;
            store_image[dst] = image;
        }
        atomicAdd(&hist[image < 0 ? 0 : evc_class(cls, n_classes)], 1);
    }
    __syncthreads();
    for (int c = tid; c <= n_classes; c += EVC_THREADS)
        if (hist[c]) atomicAdd(&counters[c == 0 ? SSDHIP_EVAL_BAD_CLASS : SSDHIP_EVAL_CLASS_COUNT + c - 1], hist[c]);
}

__global__ void evc_reset_kernel(int* __restrict__ counters) {
    for (int i = threadIdx.x; i < SSDHIP_EVAL_COUNTERS; i += blockDim.x) counters[i] = 0;
}

// ---- pack --------------------------------------------------------------------------------------------------------------------------
// the 0-based class slot of store row i, or -1 for a row the matcher has no segment for
template <typename T>
__device__ __forceinline__ int evp_slot(const T* __restrict__ store_rows, const int* __restrict__ store_image, int i, int n, int n_images,
                                        int n_classes) {
    if (i >= n) return -1;
    const int image = store_image[i];
    if (image < 0 || image >= n_images) return -1;
    return evc_class(store_rows[(size_t)i * 6], n_classes) - 1;
}

template <typename T>
__global__ __launch_bounds__(EVP_CHUNK) void evp_count_kernel(const T* __restrict__ store_rows, const int* __restrict__ store_image, int n,
                                                              int n_images, int n_classes, int n_chunks, int* __restrict__ counts) {
    __shared__ int hist[EVC_MAXC];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    for (int c = tid; c < n_classes; c += EVP_CHUNK) hist[c] = 0;
    __syncthreads();
    const int slot = evp_slot(store_rows, store_image, chunk * EVP_CHUNK + tid, n, n_images, n_classes);
    if (slot >= 0) atomicAdd(&hist[slot], 1);
    __syncthreads();
    for (int c = tid; c < n_classes; c += EVP_CHUNK) counts[(size_t)c * n_chunks + chunk] = hist[c];
}

// offsets[i] = sum of counts[0 .. i-1], i < L; offsets[L] = the total.  One workgroup, each thread a contiguous stretch.
__global__ __launch_bounds__(EVP_SCAN_THREADS) void evp_scan_kernel(const int* __restrict__ counts, int L, int* __restrict__ offsets) {
    __shared__ int wsum[EVP_SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    const int per = (L + EVP_SCAN_THREADS - 1) / EVP_SCAN_THREADS;
    const int lo = tid * per < L ? tid * per : L, hi = lo + per < L ? lo + per : L;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += counts[i];
    int total;
    int run = evc_block_exclusive(sum, wsum, EVP_SCAN_THREADS / 64, total);
    for (int i = lo; i < hi; ++i) {
        offsets[i] = run;
        run += counts[i];
    }
    if (tid == 0) offsets[L] = total;
}

template <typename T>
__global__ __launch_bounds__(EVP_CHUNK) void evp_scatter_kernel(const T* __restrict__ store_rows, const int* __restrict__ store_image, int n,
                                                                int n_images, int n_classes, int n_chunks, const int* __restrict__ offsets,
                                                                float* __restrict__ pred, int* __restrict__ segment, int* __restrict__ slot_out,
                                                                int* __restrict__ starts, int out_rows) {
    __shared__ int wcount[EVP_WAVES * EVC_MAXC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, chunk = blockIdx.x;
    if (chunk == 0)
        for (int c = tid; c <= n_classes; c += EVP_CHUNK) starts[c] = offsets[(size_t)c * n_chunks];   // c == n_classes: offsets[L]
    for (int c = tid; c < EVP_WAVES * EVC_MAXC; c += EVP_CHUNK) wcount[c] = 0;
    __syncthreads();
    const int i = chunk * EVP_CHUNK + tid;
    const int slot = evp_slot(store_rows, store_image, i, n, n_images, n_classes);
    const unsigned key = slot < 0 ? 255u : (unsigned)slot;      // slot < 128
    evc_u64 peers = ~0ull;                                      // the lanes of this wave with the same key
    for (int bit = 0; bit < 8; ++bit) {
        const bool set = (key >> bit) & 1u;
        const evc_u64 bal = __ballot(set);
        peers &= set ? bal : ~bal;
    }
    const int rank_in_wave = __popcll(peers & ((1ull << lane) - 1ull));
    if (slot >= 0) atomicAdd(&wcount[w * EVC_MAXC + slot], 1);  // counts only: the rank comes from the ballots and the sums below
    __syncthreads();
    if (slot < 0) return;
    int rank = rank_in_wave;
    for (int v = 0; v < w; ++v) rank += wcount[v * EVC_MAXC + slot];
    const int dst = offsets[(size_t)slot * n_chunks + chunk] + rank;
    if (dst < 0 || dst >= out_rows) return;
    const T* src = store_rows + (size_t)i * 6;
    float* out = pred + (size_t)dst * 5;
    out[0] = (float)src[1]; out[1] = (float)src[2]; out[2] = (float)src[3]; out[3] = (float)src[4]; out[4] = (float)src[5];
    segment[dst] = slot * n_images + store_image[i];
    slot_out[dst] = slot;
}

static inline size_t evp_align(size_t v) { return (v + 255) / 256 * 256; }
static inline int evp_chunks(int n) { return n > 0 ? (n + EVP_CHUNK - 1) / EVP_CHUNK : 1; }

// 10^n as the host's round() uses it (exact in both dtypes for n <= 9); 0 = leave the value alone
static inline double evc_pow10(int n) {
    double p = 1.0;
    for (int i = 0; i < n; ++i) p *= 10.0;
    return n > 0 ? p : 0.0;
}

template <typename T>
static int evc_collect(const void* rows_, int B, int R, const int* count, const double* desc, int n_images, int n_classes, int coord_decimals,
                       int conf_decimals, void* store_rows, int* store_image, int capacity, int* counters, int* plan, hipStream_t stream) {
    const T* rows = static_cast<const T*>(rows_);
    hipLaunchKernelGGL(evc_plan_kernel<T>, dim3(1), dim3(EVC_PLAN_THREADS), 0, stream, rows, B, R, count, capacity, counters, plan);
    if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    hipLaunchKernelGGL(evc_collect_kernel<T>, dim3(B), dim3(EVC_THREADS), 0, stream, rows, B, R, count, desc, n_images, n_classes,
                       (T)evc_pow10(coord_decimals), (T)evc_pow10(conf_decimals), static_cast<T*>(store_rows), store_image, capacity,
                       counters, (const int*)plan);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

template <typename T>
static int evp_pack(const void* store_rows_, const int* store_image, int n, int n_images, int n_classes, float* pred, int* segment, int* slot,
                    int* starts, int out_rows, int* counts, int* offsets, hipStream_t stream) {
    const T* store_rows = static_cast<const T*>(store_rows_);
    const int n_chunks = evp_chunks(n);
    hipLaunchKernelGGL(evp_count_kernel<T>, dim3(n_chunks), dim3(EVP_CHUNK), 0, stream, store_rows, store_image, n, n_images, n_classes,
                       n_chunks, counts);
    if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    hipLaunchKernelGGL(evp_scan_kernel, dim3(1), dim3(EVP_SCAN_THREADS), 0, stream, (const int*)counts, n_classes * n_chunks, offsets);
    if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    hipLaunchKernelGGL(evp_scatter_kernel<T>, dim3(n_chunks), dim3(EVP_CHUNK), 0, stream, store_rows, store_image, n, n_images, n_classes,
                       n_chunks, (const int*)offsets, pred, segment, slot, starts, out_rows);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

}  // namespace ssdhip

using namespace ssdhip;

extern "C" int ssdhip_eval_store_reset(int* counters, void* stream_) {
    if (!counters) return SSDHIP_E_BADARG;
    hipLaunchKernelGGL(evc_reset_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream_), counters);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_eval_collect(const void* rows, int dtype, int B, int R, const int* count, const double* desc, int n_images,
                                   int n_classes, int coord_decimals, int conf_decimals, void* store_rows, int* store_image, int capacity,
                                   int* counters, void* ws, size_t ws_bytes, void* stream_) {
    if (dtype != SSDHIP_F32 && dtype != SSDHIP_F64) return SSDHIP_E_BADARG;
    if (B < 1 || B > EVC_PLAN_THREADS || R < 1 || (long long)B * R > (1ll << 30)) return SSDHIP_E_BADARG;
    if (n_images < 1 || n_classes < 1 || n_classes > EVC_MAXC || capacity < 0) return SSDHIP_E_BADARG;
    if (coord_decimals < 0 || coord_decimals > 9 || conf_decimals < 0 || conf_decimals > 9) return SSDHIP_E_BADARG;
    if (!rows || !desc || !store_rows || !store_image || !counters) return SSDHIP_E_BADARG;
    if (!ws || ws_bytes < (size_t)2 * B * sizeof(int)) return SSDHIP_E_WORKSPACE;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    int* plan = static_cast<int*>(ws);
    return dtype == SSDHIP_F32
               ? evc_collect<float>(rows, B, R, count, desc, n_images, n_classes, coord_decimals, conf_decimals, store_rows, store_image,
                                    capacity, counters, plan, stream)
               : evc_collect<double>(rows, B, R, count, desc, n_images, n_classes, coord_decimals, conf_decimals, store_rows, store_image,
                                     capacity, counters, plan, stream);
}

extern "C" size_t ssdhip_eval_pack_workspace_bytes(int n, int n_classes) {
    if (n < 0 || n_classes < 1 || n_classes > EVC_MAXC) return 0;
    const size_t L = (size_t)n_classes * evp_chunks(n);
    return evp_align(L * sizeof(int)) + evp_align((L + 1) * sizeof(int));
}

extern "C" int ssdhip_eval_pack(const void* store_rows, int dtype, const int* store_image, int n, int n_images, int n_classes, float* pred,
                                int* segment, int* slot, int* starts, int out_rows, void* ws, size_t ws_bytes, void* stream_) {
    if (dtype != SSDHIP_F32 && dtype != SSDHIP_F64) return SSDHIP_E_BADARG;
    if (n < 0 || n > (1 << 30) || out_rows < 0 || n_images < 1 || n_classes < 1 || n_classes > EVC_MAXC) return SSDHIP_E_BADARG;
    if ((long long)n_classes * n_images > 0x7fffffffll) return SSDHIP_E_BADARG;
    if (!starts || (n > 0 && (!store_rows || !store_image))) return SSDHIP_E_BADARG;
    if (out_rows > 0 && (!pred || !segment || !slot)) return SSDHIP_E_BADARG;
    const size_t need = ssdhip_eval_pack_workspace_bytes(n, n_classes);
    if (!ws || ws_bytes < need) return SSDHIP_E_WORKSPACE;
    const size_t L = (size_t)n_classes * evp_chunks(n);
    int* counts = static_cast<int*>(ws);
    int* offsets = reinterpret_cast<int*>(static_cast<unsigned char*>(ws) + evp_align(L * sizeof(int)));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return dtype == SSDHIP_F32 ? evp_pack<float>(store_rows, store_image, n, n_images, n_classes, pred, segment, slot, starts, out_rows, counts,
                                                 offsets, stream)
                               : evp_pack<double>(store_rows, store_image, n, n_images, n_classes, pred, segment, slot, starts, out_rows, counts,
                                                  offsets, stream);
}
