// ssdhip_cocoeval.hip -- COCO bbox evaluation (the COCOeval protocol of ssd300_evaluation_COCO.ipynb's last cell) on gfx950 (MI355X).
//
// The protocol (restated in tests/np_cocoeval.py; pycocotools itself is not available to this project): every (image, category) pair's
// detections in descending score order (stable), cut to the largest detection cap, are walked greedily over the pair's ground truth
// once per (area range, IoU threshold); crowd boxes may be matched repeatedly, ignored ground truth sorts behind the rest and a
// detection that holds a non-ignored candidate stops at the first ignored one.  Then per (category, area range, cap, threshold) the
// category's detections in descending score order give cumulative true / false positives, the precision envelope and its value at
// the recall thresholds.  All arithmetic is IEEE double, one rounding per operation (-ffp-contract=off).
//
//   ssdhip_coco_match       sort     two stable rocPRIM radix sorts of the detections (score descending, then pair index) and one of
//                                    the ground truth (pair index); CSR offsets per pair by binary search in the sorted pair keys
//                           C1 coco_match_kernel   one wave per pair.  G <= 64 and D * G <= 1536: the D x G IoU matrix in LDS, the
//                                    ignore / crowd / matched sets as 64-bit masks in registers.  Otherwise: IoU recomputed from the boxes
//                                    in global memory, matched flags in the workspace (correct for any G, not fast).  The A * T walks of
//                                    a pair are independent: one lane each.
//   ssdhip_coco_accumulate  sort     the cut detections stably by score, then stably by category: each category's stretch is its
//                                    argsort(-score, kind='mergesort') of the pairs concatenated in image order, and the elements of
//                                    in-image rank < m are that order for cap m
//                           C2 coco_accumulate_kernel   one workgroup per (category, area range, cap, threshold): a counting pass, then a
//                                    pass from the END of the stretch carrying the suffix counts and the running maximum of the precision
//                                    (the right-to-left envelope); the c-th true positive writes the recall thresholds it is the first
//                                    to reach.  Every output element is written by exactly one workgroup: no fill pass, no atomics, no
//                                    cross-workgroup hand-off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "ssdhip.h"
#include "ssdhip_math.h"

namespace ssdhip {

constexpr int COCO_THREADS = 256;
constexpr int COCO_WAVE = 64;
constexpr int COCO_LDS_IOU = 1536;       // D * G doubles kept in LDS (12 KB per wave)
constexpr int COCO_MAX_T = 32, COCO_MAX_A = 8, COCO_MAX_M = 8, COCO_MAX_R = 1024;

// order-preserving map double -> u64, inverted: ascending keys == descending scores; -0.0 and +0.0 share a key (as -score compares)
__device__ __forceinline__ u64 coco_desc_key(double s) {
    s = s + 0.0;
    const u64 u = (u64)__double_as_longlong(s);
    const u64 k = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
    return ~k;
}

// keys[i] = descending-score key of score[src[i]] (src NULL: identity); idx[i] = i
__global__ __launch_bounds__(COCO_THREADS) void coco_score_keys_kernel(int n, const double* __restrict__ score, const int* __restrict__ src,
                                                                       u64* __restrict__ keys, int* __restrict__ idx) {
    const int i = blockIdx.x * COCO_THREADS + threadIdx.x;
    if (i >= n) return;
    keys[i] = coco_desc_key(score[src ? src[i] : i]);
    idx[i] = i;
}

// keys[i] = pair[src[i]] (src NULL: identity); idx[i] = i when idx is given
__global__ __launch_bounds__(COCO_THREADS) void coco_gather_keys_kernel(int n, const int* __restrict__ pair, const int* __restrict__ src,
                                                                        u32* __restrict__ keys, int* __restrict__ idx) {
    const int i = blockIdx.x * COCO_THREADS + threadIdx.x;
    if (i >= n) return;
    keys[i] = (u32)pair[src ? src[i] : i];
    if (idx) idx[i] = i;
}

// offsets[s] = first position of the sorted keys that is >= s, for s = 0 .. n_seg
__global__ __launch_bounds__(COCO_THREADS) void coco_offsets_kernel(int n, const u32* __restrict__ sorted_keys, int n_seg, int* __restrict__ offsets) {
    const int s = blockIdx.x * COCO_THREADS + threadIdx.x;
    if (s > n_seg) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted_keys[mid] < (u32)s) lo = mid + 1; else hi = mid;
    }
    offsets[s] = lo;
}

// IoU of a detection and a ground-truth box, both [x, y, w, h]; a crowd box divides by the detection's area
__device__ __forceinline__ double coco_iou(const double* __restrict__ d, const double* __restrict__ g, bool crowd) {
    const double da = d[2] * d[3];
    const double ga = g[2] * g[3];
    const double dx1 = d[0] + d[2], gx1 = g[0] + g[2];
    const double w = (dx1 < gx1 ? dx1 : gx1) - (d[0] > g[0] ? d[0] : g[0]);
    if (w <= 0.0) return 0.0;
    const double dy1 = d[1] + d[3], gy1 = g[1] + g[3];
    const double h = (dy1 < gy1 ? dy1 : gy1) - (d[1] > g[1] ? d[1] : g[1]);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : (da + ga) - i;
    return i / u;
}

struct CocoMatchArgs {
    const double* det_box;
    const double* gt_box;
    const double* gt_area;
    const unsigned char* gt_crowd;
    const double* iou_thrs;
    const double* area_rng;
    const int* det_order;
    const int* det_offsets;
    const int* gt_order;
    const int* gt_offsets;
    int* det_match;
    unsigned char* gt_ignore;
    int* pair_npig;
    unsigned char* gt_matched;      // workspace [A * T, n_gt]: the walk's "matched" flags of pairs that do not fit LDS
    int n_det, n_gt, n_pairs, T, A, max_det;
};

// det_match code: (index + 1 of the matched ground truth in the pair's input order) << 1 | ignore flag
__global__ __launch_bounds__(COCO_WAVE) void coco_match_kernel(CocoMatchArgs q) {
    __shared__ double s_iou[COCO_LDS_IOU];
    __shared__ u64 s_ign[COCO_MAX_A];
    const int pair = blockIdx.x;
    const int lane = threadIdx.x;
    const int d0 = q.det_offsets[pair], g0 = q.gt_offsets[pair];
    int D = q.det_offsets[pair + 1] - d0;
    const int G = q.gt_offsets[pair + 1] - g0;
    if (D > q.max_det) D = q.max_det;
    const int W = q.A * q.T;

    // ignore flags per (area range, ground truth) and the pair's count of non-ignored ground truth
    for (int a = 0; a < q.A; ++a) {
        const double lo = q.area_rng[2 * a], hi = q.area_rng[2 * a + 1];
        int n = 0;
        for (int g = lane; g < G; g += COCO_WAVE) {
            const int src = q.gt_order[g0 + g];
            const double ar = q.gt_area[src];
            const bool ign = q.gt_crowd[src] != 0 || ar < lo || ar > hi;
            q.gt_ignore[(size_t)a * q.n_gt + g0 + g] = ign ? 1 : 0;
            n += ign ? 0 : 1;
        }
        for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
        if (lane == 0) q.pair_npig[(size_t)pair * q.A + a] = n;
    }
    if (D == 0) return;

    const bool fits = G <= 64 && D * G <= COCO_LDS_IOU;
    if (fits) {
        u64 crowd_mask = 0;
        {
            bool c = false;
            if (lane < G) c = q.gt_crowd[q.gt_order[g0 + lane]] != 0;
            crowd_mask = __ballot(c);
            for (int a = 0; a < q.A; ++a) {
                bool ign = false;
                if (lane < G) {
                    const double ar = q.gt_area[q.gt_order[g0 + lane]];
                    ign = c || ar < q.area_rng[2 * a] || ar > q.area_rng[2 * a + 1];
                }
                const u64 m = __ballot(ign);
                if (lane == 0) s_ign[a] = m;
            }
        }
        for (int e = lane; e < D * G; e += COCO_WAVE) {
            const int d = e / G, g = e - d * G;
            const int gs = q.gt_order[g0 + g];
            s_iou[e] = coco_iou(q.det_box + (size_t)q.det_order[d0 + d] * 4, q.gt_box + (size_t)gs * 4, q.gt_crowd[gs] != 0);
        }
        __syncthreads();
        const u64 all = G == 64 ? ~0ull : ((1ull << G) - 1ull);
        for (int w = lane; w < W; w += COCO_WAVE) {
            const int a = w / q.T, t = w - a * q.T;
            const double lo = q.area_rng[2 * a], hi = q.area_rng[2 * a + 1];
            const double thr = q.iou_thrs[t];
            const double start = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
            const u64 ign_mask = s_ign[a] & all;
            u64 matched = 0;
            int* out = q.det_match + (size_t)w * q.n_det + d0;
            for (int d = 0; d < D; ++d) {
                double best = start;
                int m = -1;
                // non-ignored ground truth in input order, then (only while no non-ignored candidate is held) the ignored ones
                u64 cand = ~ign_mask & all & ~(matched & ~crowd_mask);
                while (cand) {
                    const int g = __ffsll((unsigned long long)cand) - 1;
                    cand &= cand - 1;
                    const double v = s_iou[d * G + g];
                    if (v < best) continue;
                    best = v;
                    m = g;
                }
                if (m < 0) {
                    cand = ign_mask & ~(matched & ~crowd_mask);
                    while (cand) {
                        const int g = __ffsll((unsigned long long)cand) - 1;
                        cand &= cand - 1;
                        const double v = s_iou[d * G + g];
                        if (v < best) continue;
                        best = v;
                        m = g;
                    }
                }
                int code;
                if (m >= 0) {
                    matched |= 1ull << m;
                    code = ((m + 1) << 1) | (int)((ign_mask >> m) & 1ull);
                } else {
                    const double* b = q.det_box + (size_t)q.det_order[d0 + d] * 4;
                    const double da = b[2] * b[3];
                    code = (da < lo || da > hi) ? 1 : 0;
                }
                out[d] = code;
            }
        }
        return;
    }

    // any G: IoU from the boxes, matched flags in the workspace (each lane clears and reads only its own walks' rows)
    for (int w = lane; w < W; w += COCO_WAVE) {
        const int a = w / q.T, t = w - a * q.T;
        const double lo = q.area_rng[2 * a], hi = q.area_rng[2 * a + 1];
        const double thr = q.iou_thrs[t];
        const double start = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
        unsigned char* matched = q.gt_matched + (size_t)w * q.n_gt + g0;
        for (int g = 0; g < G; ++g) matched[g] = 0;
        int* out = q.det_match + (size_t)w * q.n_det + d0;
        for (int d = 0; d < D; ++d) {
            const double* db = q.det_box + (size_t)q.det_order[d0 + d] * 4;
            double best = start;
            int m = -1;
            for (int pass = 0; pass < 2; ++pass) {
                if (pass == 1 && m >= 0) break;                     // holding a non-ignored candidate: stop at the first ignored one
                for (int g = 0; g < G; ++g) {
                    const int gs = q.gt_order[g0 + g];
                    const double ar = q.gt_area[gs];
                    const bool crowd = q.gt_crowd[gs] != 0;
                    const bool ig = crowd || ar < lo || ar > hi;
                    if ((int)ig != pass) continue;
                    if (matched[g] && !crowd) continue;
                    const double v = coco_iou(db, q.gt_box + (size_t)gs * 4, crowd);
                    if (v < best) continue;
                    best = v;
                    m = g;
                }
            }
            int code;
            if (m >= 0) {
                matched[m] = 1;
                const int gs = q.gt_order[g0 + m];
                const double ar = q.gt_area[gs];
                const bool ig = q.gt_crowd[gs] != 0 || ar < lo || ar > hi;
                code = ((m + 1) << 1) | (ig ? 1 : 0);
            } else {
                const double da = db[2] * db[3];
                code = (da < lo || da > hi) ? 1 : 0;
            }
            out[d] = code;
        }
    }
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------------
// category key of the j-th element of the score-sorted sequence: K (behind every category) for a detection past the cut
__global__ __launch_bounds__(COCO_THREADS) void coco_acc_cat_keys_kernel(int n, const int* __restrict__ by_score, const int* __restrict__ det_pair,
                                                                         const int* __restrict__ det_order, const int* __restrict__ det_offsets,
                                                                         int n_images, int K, int max_det, u32* __restrict__ keys) {
    const int j = blockIdx.x * COCO_THREADS + threadIdx.x;
    if (j >= n) return;
    const int s = by_score[j];
    const int pair = det_pair[det_order[s]];
    const int rank = s - det_offsets[pair];
    keys[j] = rank < max_det ? (u32)(pair / n_images) : (u32)K;
}

// per element j of the category-sorted sequence: its in-image rank and its score, so the accumulation reads them in order
__global__ __launch_bounds__(COCO_THREADS) void coco_acc_rank_kernel(int n, const int* __restrict__ by_cat, const int* __restrict__ det_pair,
                                                                     const int* __restrict__ det_order, const int* __restrict__ det_offsets,
                                                                     const double* __restrict__ score, int* __restrict__ rank_of,
                                                                     double* __restrict__ score_of) {
    const int j = blockIdx.x * COCO_THREADS + threadIdx.x;
    if (j >= n) return;
    const int s = by_cat[j];
    const int src = det_order[s];
    rank_of[j] = s - det_offsets[det_pair[src]];
    score_of[j] = score[src];
}

struct CocoAccArgs {
    const int* rank_of;         // [n_det] by element of the category-sorted sequence
    const double* score_of;
    const int* det_match;
    const int* pair_npig;
    const int* max_dets;
    const double* rec_thrs;
    const int* by_cat;          // positions s, category by category, each stretch in descending score order (stable)
    const int* cat_offsets;     // [K + 2]
    double* precision;
    double* recall;
    double* scores;
    int n_det, n_images, K, T, A, M, R;
};

template <typename V, typename Op>
__device__ __forceinline__ V coco_block_scan(V v, V* buf, Op op) {            // inclusive, over threadIdx.x; buf: COCO_THREADS values
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < COCO_THREADS; off <<= 1) {
        V o = v;
        if (tid >= off) o = op(buf[tid - off], v);
        __syncthreads();
        v = o;
        buf[tid] = v;
        __syncthreads();
    }
    return v;
}

struct CocoSumOp { __device__ u64 operator()(u64 a, u64 b) const { return a + b; } };
struct CocoMaxOp { __device__ double operator()(double a, double b) const { return a > b ? a : b; } };
struct CocoMinOp { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };

__global__ __launch_bounds__(COCO_THREADS) void coco_accumulate_kernel(CocoAccArgs q) {
    __shared__ int s_need[COCO_MAX_R];           // the true-positive count at which recall first reaches rec_thrs[r]
    __shared__ u64 s_scan[COCO_THREADS];
    __shared__ double s_max[COCO_THREADS];
    __shared__ int s_min[COCO_THREADS];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int t = b % q.T; b /= q.T;
    const int m = b % q.M; b /= q.M;
    const int a = b % q.A; b /= q.A;
    const int k = b;
    const int cap = q.max_dets[m];
    const size_t AM = (size_t)q.A * q.M;
    const size_t out_rec = ((size_t)t * q.K + k) * AM + (size_t)a * q.M + m;
#define COCO_OUT(r) ((((size_t)t * q.R + (r)) * q.K + k) * AM + (size_t)a * q.M + m)

    // non-ignored ground truth of (k, a) over the images
    u64 part = 0;
    for (int i = tid; i < q.n_images; i += COCO_THREADS) part += (u64)q.pair_npig[((size_t)k * q.n_images + i) * q.A + a];
    coco_block_scan<u64>(part, s_scan, CocoSumOp());
    __syncthreads();
    const int npig = (int)s_scan[COCO_THREADS - 1];
    __syncthreads();
    if (npig == 0) {
        for (int r = tid; r < q.R; r += COCO_THREADS) { q.precision[COCO_OUT(r)] = -1.0; q.scores[COCO_OUT(r)] = -1.0; }
        if (tid == 0) q.recall[out_rec] = -1.0;
        return;
    }
    const double npig_d = (double)npig;
    for (int r = tid; r < q.R; r += COCO_THREADS) {                 // smallest c with (double)c / npig >= rec_thrs[r]; npig + 1: never
        const double thr = q.rec_thrs[r];
        int lo = 0, hi = npig + 1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((double)mid / npig_d >= thr) hi = mid; else lo = mid + 1;
        }
        s_need[r] = lo;
    }
    __syncthreads();

    const int j0 = q.cat_offsets[k], j1 = q.cat_offsets[k + 1];
    const int* codes = q.det_match + ((size_t)a * q.T + t) * q.n_det;

    // pass 1: totals, and the first element that takes part under this cap
    u64 cnt = 0;                                                     // true positives << 32 | false positives
    int first = 0x7fffffff;
    for (int j = j0 + tid; j < j1; j += COCO_THREADS) {
        if (q.rank_of[j] >= cap) continue;
        if (j < first) first = j;
        const int code = codes[q.by_cat[j]];
        if (!(code & 1)) cnt += (code >> 1) ? (1ull << 32) : 1ull;
    }
    coco_block_scan<u64>(cnt, s_scan, CocoSumOp());
    const u64 tot = s_scan[COCO_THREADS - 1];
    coco_block_scan<int>(first, s_min, CocoMinOp());
    first = s_min[COCO_THREADS - 1];
    __syncthreads();
    const int tp_tot = (int)(tot >> 32), fp_tot = (int)(tot & 0xffffffffull);

    if (first == 0x7fffffff) {                                       // no detections: recall 0, precision and scores 0
        for (int r = tid; r < q.R; r += COCO_THREADS) { q.precision[COCO_OUT(r)] = 0.0; q.scores[COCO_OUT(r)] = 0.0; }
        if (tid == 0) q.recall[out_rec] = 0.0;
        return;
    }
    if (tid == 0) q.recall[out_rec] = (double)tp_tot / npig_d;
    for (int r = tid; r < q.R; r += COCO_THREADS)                    // thresholds the sequence never reaches
        if (s_need[r] > tp_tot) { q.precision[COCO_OUT(r)] = 0.0; q.scores[COCO_OUT(r)] = 0.0; }

    // pass 2, from the end: thread tid of a chunk takes element hi - 1 - tid, so a scan over tid is a suffix scan over the elements
    u64 after = 0;                                                   // counts behind the chunk
    double env = 0.0;                                                // running maximum of the precision behind the chunk
    const double eps = 2.220446049250313e-16;                        // np.spacing(1)
    for (int hi = j1; hi > j0; hi -= COCO_THREADS) {
        const int j = hi - 1 - tid;
        u64 c = 0;
        bool is_tp = false;
        if (j >= j0 && q.rank_of[j] < cap) {
            const int code = codes[q.by_cat[j]];
            if (!(code & 1)) { is_tp = (code >> 1) != 0; c = is_tp ? (1ull << 32) : 1ull; }
        }
        const u64 incl = coco_block_scan<u64>(c, s_scan, CocoSumOp());
        const u64 chunk_tot = s_scan[COCO_THREADS - 1];
        const u64 behind = after + (incl - c);                       // counts strictly behind this element
        const int tp = tp_tot - (int)(behind >> 32);                 // cumulative counts at this element (inclusive)
        const int fp = fp_tot - (int)(behind & 0xffffffffull);
        double pr = 0.0;
        if (is_tp) pr = (double)tp / (((double)fp + (double)tp) + eps);
        double e = coco_block_scan<double>(pr, s_max, CocoMaxOp());
        const double chunk_max = s_max[COCO_THREADS - 1];
        e = e > env ? e : env;
        if (is_tp) {                                                 // the tp-th true positive: first to reach every r with need == tp
            const double sc = q.score_of[j];
            int lo = 0, hi_r = q.R;
            while (lo < hi_r) {                                      // rec_thrs is non-decreasing, so is s_need
                const int mid = lo + ((hi_r - lo) >> 1);
                if (s_need[mid] < tp) lo = mid + 1; else hi_r = mid;
            }
            for (int r = lo; r < q.R && s_need[r] == tp; ++r) { q.precision[COCO_OUT(r)] = e; q.scores[COCO_OUT(r)] = sc; }
        }
        __syncthreads();
        after += chunk_tot;
        env = chunk_max > env ? chunk_max : env;
    }
    // thresholds reached before any true positive (recall threshold 0): position 0 of the sequence
    {
        const double sc = q.score_of[first];
        for (int r = tid; r < q.R; r += COCO_THREADS)
            if (s_need[r] == 0) { q.precision[COCO_OUT(r)] = env; q.scores[COCO_OUT(r)] = sc; }
    }
#undef COCO_OUT
}

struct CocoWs {
    size_t keys64, keys64_out, keys32, keys32_out, idx, idx_out, gt_matched, tmp, tmp_bytes, total;
};

static inline size_t coco_align(size_t v) { return (v + 255) / 256 * 256; }

static CocoWs coco_layout(int n_det, int n_gt, int AT) {
    const size_t n = (size_t)(n_det > n_gt ? n_det : n_gt) + 1;
    size_t sort_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (u64*)nullptr, (u64*)nullptr, (int*)nullptr, (int*)nullptr, n, 0, 64, (hipStream_t)0);
    CocoWs w;
    size_t o = 0;
    w.keys64 = o;     o = coco_align(o + n * sizeof(u64));
    w.keys64_out = o; o = coco_align(o + n * sizeof(u64));
    w.keys32 = o;     o = coco_align(o + n * sizeof(u32));
    w.keys32_out = o; o = coco_align(o + n * sizeof(u32));
    w.idx = o;        o = coco_align(o + n * sizeof(int));
    w.idx_out = o;    o = coco_align(o + n * sizeof(int));
    w.gt_matched = o; o = coco_align(o + (size_t)AT * ((size_t)n_gt + 1));
    w.tmp = o;
    w.tmp_bytes = sort_bytes;
    const size_t floor_bytes = n * 32 + (1u << 20);    // never below a generous bound (the size query needs a device to answer)
    if (w.tmp_bytes < floor_bytes) w.tmp_bytes = floor_bytes;
    o = coco_align(o + w.tmp_bytes);
    w.total = o;
    return w;
}

static inline int coco_bits(unsigned v) {               // bits needed to hold the values 0 .. v
    int b = 1;
    while (b < 32 && (v >> b)) ++b;
    return b;
}

static inline int coco_blocks(int n) { return (n + COCO_THREADS - 1) / COCO_THREADS; }

}  // namespace ssdhip

using namespace ssdhip;

extern "C" size_t ssdhip_coco_match_workspace_bytes(int n_det, int n_gt, int T, int A) {
    if (n_det < 0 || n_gt < 0 || T < 1 || A < 1 || T > COCO_MAX_T || A > COCO_MAX_A) return 0;
    return coco_layout(n_det, n_gt, T * A).total;
}

extern "C" int ssdhip_coco_match(const int* det_pair, const double* det_box, const double* det_score, int n_det, const int* gt_pair,
                                 const double* gt_box, const double* gt_area, const unsigned char* gt_crowd, int n_gt, int n_pairs,
                                 const double* iou_thrs, int T, const double* area_rng, int A, int max_det, int* det_order,
                                 int* det_offsets, int* gt_order, int* gt_offsets, int* det_match, unsigned char* gt_ignore,
                                 int* pair_npig, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_det < 0 || n_gt < 0 || n_pairs < 1 || T < 1 || T > COCO_MAX_T || A < 1 || A > COCO_MAX_A || max_det < 1) return SSDHIP_E_BADARG;
    if (!iou_thrs || !area_rng || !det_order || !det_offsets || !gt_order || !gt_offsets || !det_match || !gt_ignore || !pair_npig)
        return SSDHIP_E_BADARG;
    if (n_det > 0 && (!det_pair || !det_box || !det_score)) return SSDHIP_E_BADARG;
    if (n_gt > 0 && (!gt_pair || !gt_box || !gt_area || !gt_crowd)) return SSDHIP_E_BADARG;
    const CocoWs lay = coco_layout(n_det, n_gt, T * A);
    if (!ws || ws_bytes < lay.total) return SSDHIP_E_WORKSPACE;
    unsigned char* base = static_cast<unsigned char*>(ws);
    u64* keys64 = reinterpret_cast<u64*>(base + lay.keys64);
    u64* keys64_out = reinterpret_cast<u64*>(base + lay.keys64_out);
    u32* keys32 = reinterpret_cast<u32*>(base + lay.keys32);
    u32* keys32_out = reinterpret_cast<u32*>(base + lay.keys32_out);
    int* idx = reinterpret_cast<int*>(base + lay.idx);
    int* idx_out = reinterpret_cast<int*>(base + lay.idx_out);
    void* tmp = base + lay.tmp;
    const int pair_bits = coco_bits((unsigned)n_pairs);
    size_t tmp_bytes;

    if (n_det > 0) {
        hipLaunchKernelGGL(coco_score_keys_kernel, dim3(coco_blocks(n_det)), dim3(COCO_THREADS), 0, stream, n_det, det_score, (const int*)nullptr,
                           keys64, idx);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
        tmp_bytes = lay.tmp_bytes;
        if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys64, keys64_out, idx, idx_out, (size_t)n_det, 0, 64, stream) != hipSuccess)
            return SSDHIP_E_LAUNCH;
        hipLaunchKernelGGL(coco_gather_keys_kernel, dim3(coco_blocks(n_det)), dim3(COCO_THREADS), 0, stream, n_det, det_pair, (const int*)idx_out,
                           keys32, (int*)nullptr);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
        tmp_bytes = lay.tmp_bytes;
        if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys32, keys32_out, idx_out, det_order, (size_t)n_det, 0, pair_bits, stream) != hipSuccess)
            return SSDHIP_E_LAUNCH;
    }
    hipLaunchKernelGGL(coco_offsets_kernel, dim3(coco_blocks(n_pairs + 1)), dim3(COCO_THREADS), 0, stream, n_det, (const u32*)keys32_out, n_pairs,
                       det_offsets);
    if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    if (n_gt > 0) {
        hipLaunchKernelGGL(coco_gather_keys_kernel, dim3(coco_blocks(n_gt)), dim3(COCO_THREADS), 0, stream, n_gt, gt_pair, (const int*)nullptr,
                           keys32, idx);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
        tmp_bytes = lay.tmp_bytes;
        if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys32, keys32_out, idx, gt_order, (size_t)n_gt, 0, pair_bits, stream) != hipSuccess)
            return SSDHIP_E_LAUNCH;
    }
    hipLaunchKernelGGL(coco_offsets_kernel, dim3(coco_blocks(n_pairs + 1)), dim3(COCO_THREADS), 0, stream, n_gt, (const u32*)keys32_out, n_pairs,
                       gt_offsets);
    if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;

    CocoMatchArgs q;
    q.det_box = det_box; q.gt_box = gt_box; q.gt_area = gt_area; q.gt_crowd = gt_crowd; q.iou_thrs = iou_thrs; q.area_rng = area_rng;
    q.det_order = det_order; q.det_offsets = det_offsets; q.gt_order = gt_order; q.gt_offsets = gt_offsets;
    q.det_match = det_match; q.gt_ignore = gt_ignore; q.pair_npig = pair_npig;
    q.gt_matched = base + lay.gt_matched;
    q.n_det = n_det; q.n_gt = n_gt; q.n_pairs = n_pairs; q.T = T; q.A = A; q.max_det = max_det;
    hipLaunchKernelGGL(coco_match_kernel, dim3(n_pairs), dim3(COCO_WAVE), 0, stream, q);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" size_t ssdhip_coco_accumulate_workspace_bytes(int n_det, int K) {
    if (n_det < 0 || K < 1) return 0;
    return coco_layout(n_det, 0, 0).total + coco_align(((size_t)K + 2) * sizeof(int));
}

extern "C" int ssdhip_coco_accumulate(const int* det_pair, const double* det_score, const int* det_order, const int* det_offsets, int n_det,
                                      const int* det_match, const int* pair_npig, int n_images, int K, int T, int A, const int* max_dets,
                                      int M, int max_det, const double* rec_thrs, int R, double* precision, double* recall,
                                      double* scores, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_det < 0 || n_images < 1 || K < 1 || T < 1 || T > COCO_MAX_T || A < 1 || A > COCO_MAX_A || M < 1 || M > COCO_MAX_M || R < 1 ||
        R > COCO_MAX_R || max_det < 1)
        return SSDHIP_E_BADARG;
    if ((long long)K * T * A * M > 0x7fffffffLL) return SSDHIP_E_BADARG;
    if (!det_offsets || !pair_npig || !max_dets || !rec_thrs || !precision || !recall || !scores) return SSDHIP_E_BADARG;
    if (n_det > 0 && (!det_pair || !det_score || !det_order || !det_match)) return SSDHIP_E_BADARG;
    const CocoWs lay = coco_layout(n_det, 0, 0);
    const size_t need = lay.total + coco_align(((size_t)K + 2) * sizeof(int));
    if (!ws || ws_bytes < need) return SSDHIP_E_WORKSPACE;
    unsigned char* base = static_cast<unsigned char*>(ws);
    u64* keys64 = reinterpret_cast<u64*>(base + lay.keys64);
    u64* keys64_out = reinterpret_cast<u64*>(base + lay.keys64_out);
    u32* keys32 = reinterpret_cast<u32*>(base + lay.keys32);
    u32* keys32_out = reinterpret_cast<u32*>(base + lay.keys32_out);
    int* idx = reinterpret_cast<int*>(base + lay.idx);
    int* idx_out = reinterpret_cast<int*>(base + lay.idx_out);
    void* tmp = base + lay.tmp;
    int* cat_offsets = reinterpret_cast<int*>(base + lay.total);
    size_t tmp_bytes;

    if (n_det > 0) {
        // per sorted position s of ssdhip_coco_match's det_order: the descending-score key and s
        hipLaunchKernelGGL(coco_score_keys_kernel, dim3(coco_blocks(n_det)), dim3(COCO_THREADS), 0, stream, n_det, det_score, det_order, keys64, idx);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
        tmp_bytes = lay.tmp_bytes;
        if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys64, keys64_out, idx, idx_out, (size_t)n_det, 0, 64, stream) != hipSuccess)
            return SSDHIP_E_LAUNCH;
        hipLaunchKernelGGL(coco_acc_cat_keys_kernel, dim3(coco_blocks(n_det)), dim3(COCO_THREADS), 0, stream, n_det, (const int*)idx_out, det_pair,
                           det_order, det_offsets, n_images, K, max_det, keys32);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
        tmp_bytes = lay.tmp_bytes;
        if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys32, keys32_out, idx_out, idx, (size_t)n_det, 0, coco_bits((unsigned)K), stream) !=
            hipSuccess)
            return SSDHIP_E_LAUNCH;
    }
    hipLaunchKernelGGL(coco_offsets_kernel, dim3(coco_blocks(K + 2)), dim3(COCO_THREADS), 0, stream, n_det, (const u32*)keys32_out, K + 1,
                       cat_offsets);
    if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    int* rank_of = reinterpret_cast<int*>(keys64);                  // the sorts are done: their key buffers carry the two tables
    double* score_of = reinterpret_cast<double*>(keys64_out);
    if (n_det > 0) {
        hipLaunchKernelGGL(coco_acc_rank_kernel, dim3(coco_blocks(n_det)), dim3(COCO_THREADS), 0, stream, n_det, (const int*)idx, det_pair,
                           det_order, det_offsets, det_score, rank_of, score_of);
        if (hipGetLastError() != hipSuccess) return SSDHIP_E_LAUNCH;
    }

    CocoAccArgs q;
    q.rank_of = rank_of; q.score_of = score_of; q.det_match = det_match;
    q.pair_npig = pair_npig; q.max_dets = max_dets; q.rec_thrs = rec_thrs; q.by_cat = idx; q.cat_offsets = cat_offsets;
    q.precision = precision; q.recall = recall; q.scores = scores;
    q.n_det = n_det; q.n_images = n_images; q.K = K; q.T = T; q.A = A; q.M = M; q.R = R;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(K * A * M * T)), dim3(COCO_THREADS), 0, stream, q);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
