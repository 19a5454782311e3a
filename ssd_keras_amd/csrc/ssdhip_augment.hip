// ssdhip_augment.hip -- the DECISIONS of the original-SSD augmentation chain for a whole batch in one launch, gfx950 (MI355X).
//
// Replaces, for a device-resident batch, the per-image Python loop over (reference data_generator/)
//   data_augmentation_chain_original_ssd.py:103-162  SSDExpand        (RandomPatch, prob 0.5, canvas 1-4 x the image)
//   data_augmentation_chain_original_ssd.py:29-101   SSDRandomCrop    (RandomPatchInf: rounds of 50 candidate patches, IoU-validated)
//   object_detection_2d_geometric_ops.py:202-262     RandomFlip, :86-148 ResizeRandomInterp + Resize's label arithmetic
//   object_detection_2d_patch_sampling_ops.py:24-339 PatchCoordinateGenerator, CropPad (label shift, centre-point BoxFilter, clipping)
//   object_detection_2d_image_boxes_validation_utils.py:79-322  BoxFilter / ImageValidator
// i.e. everything of SSDDataAugmentation.__call__ (:208-280) behind the photometric part that is not a pixel operation.  Round 4 ran
// it per image on the host with one GPU round trip per sampling round (733 images/s for a pipeline whose two pixel kernels take 0.4 ms
// per batch of 32); here one WAVE per image walks the chain:
//   * the random numbers are NumPy's: the image's MT19937 state (np.random.RandomState(seed).get_state(), after the photometric draws the
//     host still makes) lives in LDS, and uniform / randint / choice consume it exactly as numpy/random/mtrand does (53-bit doubles from
//     two words, masked rejection sampling for bounded integers, searchsorted over the normalised cumulative weights) -- the decisions,
//     and the stream position afterwards, are those of the per-image chain under the same seed, bit for bit (tests/test_image_ops.py);
//   * a candidate patch is validated by the lanes in parallel (lane = ground truth box, IoU in the reference's float64 expression) and the
//     search stops at the first valid trial, which is where the reference's loop stops consuming random numbers;
//   * the label arithmetic (shift, centre-point filter, clipping, mirroring, rounding to the network input, degenerate-box filter) runs in
//     float64, exact for int64 and float64 label arrays alike.
// Outputs per image: the geometry (canvas, crop window, flip, interpolation mode) the gather launch needs, the surviving labels, and the
// generator state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssdhip.h"
#include "ssdhip_math.h"

namespace ssdhip {

constexpr int AUG_MAXG = 64;                              // ground truth boxes per image (one lane each)

struct AugParams {
    int H, W;                                             // the batch's image size
    double exp_prob, exp_min, exp_max;                    // SSDExpand: RandomPatch(prob), PatchCoordinateGenerator(min_scale, max_scale, scale_uniformly)
    double crop_prob, crop_min, crop_max, ar_min, ar_max; // SSDRandomCrop: RandomPatchInf(prob), generator scales / aspect ratios
    int n_trials, n_bounds;
    double cdf[8], lower[8], upper[8];                    // BoundGenerator: cumulative weights / cdf[-1] (as np.random.choice builds them), bounds
    double flip_prob;
    int n_modes, modes[8], out_h, out_w;                  // ResizeRandomInterp
    int max_rounds;                                       // safety net of the crop loop (the reference loops without one)
};

struct Mt {                                               // numpy's rk_state: 624 key words in LDS, the position in a register
    u32* key;
    int pos;
    // Round 6: a window of 64 TEMPERED outputs in a register, lane i = output `base + i`.  A draw is then one v_readlane with a scalar
    // index instead of a dependent LDS round trip + the tempering ALU chain -- the batch-serial walk of ssd_augment_stream_kernel is a
    // chain of ~100-cycle draws otherwise (1.2 ms for a batch of 32).  base < 0: no window loaded.
    u32 win;
    int base;
};

__device__ __forceinline__ void mt_twist(u32* key, int lane) {
    constexpr u32 UP = 0x80000000u, LO = 0x7fffffffu, MAG = 0x9908b0dfu;
    for (int base = 0; base < 623; base += 64) {
        const int i = base + lane;
        u32 nv = 0u;
        if (i < 623) {
            const u32 y = (key[i] & UP) | (key[i + 1] & LO);
            const u32 c = key[i < 227 ? i + 397 : i - 227];
            nv = c ^ (y >> 1) ^ ((y & 1u) ? MAG : 0u);
        }
        __syncthreads();                                  // every lane has read before any lane writes (one wave per block)
        if (i < 623) key[i] = nv;
        __syncthreads();
    }
    if (lane == 0) {
        const u32 y = (key[623] & UP) | (key[0] & LO);
        key[623] = key[396] ^ (y >> 1) ^ ((y & 1u) ? MAG : 0u);
    }
    __syncthreads();
}

__device__ __forceinline__ u32 mt_u32(Mt& s, int lane) {
    if (s.pos == 624) { mt_twist(s.key, lane); s.pos = 0; s.base = -1; }
    if (s.base < 0 || s.pos - s.base >= 64) {            // (the position only moves forward inside a block of 624)
        s.base = s.pos;
        const int i = s.pos + lane;
        u32 y = s.key[i < 624 ? i : 623];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        s.win = y;
    }
    const int k = __builtin_amdgcn_readfirstlane(s.pos - s.base);
    ++s.pos;
    return (u32)__builtin_amdgcn_readlane((int)s.win, k);
}
__device__ __forceinline__ double mt_double(Mt& s, int lane) {           // rk_double / random_sample
    const u32 a = mt_u32(s, lane) >> 5, b = mt_u32(s, lane) >> 6;
    return ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0);   // (x 2^-53: exact, the same double as NumPy's division)
}
__device__ __forceinline__ double mt_uniform(Mt& s, int lane, double lo, double hi) { return lo + (hi - lo) * mt_double(s, lane); }
// np.random.randint(lo, hi) for int64 results: masked rejection sampling on 32-bit words (numpy/random/_bounded_integers: use_masked)
__device__ __forceinline__ long long mt_randint(Mt& s, int lane, long long lo, long long hi) {
    const unsigned long long rng = (unsigned long long)(hi - 1 - lo);
    if (rng == 0ull) return lo;
    unsigned long long mask = rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16; mask |= mask >> 32;
    if (rng == 0xffffffffull) return lo + (long long)mt_u32(s, lane);
    if (rng > 0xffffffffull) {                                          // (never in this chain: extents are image sizes)
        unsigned long long v;
        do { const unsigned long long hi32 = mt_u32(s, lane), lo32 = mt_u32(s, lane); v = ((hi32 << 32) | lo32) & mask; } while (v > rng);
        return lo + (long long)v;
    }
    u32 v;
    do { v = mt_u32(s, lane) & (u32)mask; } while (v > (u32)rng);
    return lo + (long long)v;
}
// PatchCoordinateGenerator._position (object_detection_2d_patch_sampling_ops.py:163-178)
__device__ __forceinline__ int aug_position(Mt& s, int lane, int extent, int size) {
    const int room = extent - size;
    return (int)(room >= 0 ? mt_randint(s, lane, 0, (long long)room + 1) : mt_randint(s, lane, room, 1));
}

// The geometric decisions of ONE image (SSDExpand, SSDRandomCrop, RandomFlip, ResizeRandomInterp + the label arithmetic) by one wave on
// the generator state `s`: what SSDDataAugmentation.__call__ does behind the photometric part (:208-280).  (H0, W0): the image's size.
__device__ __forceinline__ void aug_decide_image(const AugParams& p, Mt& s, const int lane, const int b, const int H0, const int W0,
                                                 const double* __restrict__ lab_in,
                                                 const int* __restrict__ n_in, int* __restrict__ geo, double* __restrict__ lab_out,
                                                 int* __restrict__ n_out) {
    const int n = n_in[b];
    bool alive = lane < n;
    double cls = 0.0, x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;
    if (alive) {
        const double* r = lab_in + ((size_t)b * AUG_MAXG + lane) * 5;
        cls = r[0]; x0 = r[1]; y0 = r[2]; x1 = r[3]; y1 = r[4];
    }
    int H = H0, W = W0;
    int g[12] = {0, 0, 0, H, W, 0, 0, 0, H, W, 0, 0};

    // ---- SSDExpand: RandomPatch(prob), one trial, no validator: the image on a canvas of 1 .. 4 times its size ----------------------
    if (!(mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.exp_prob))) {
        const double factor = mt_uniform(s, lane, p.exp_min, p.exp_max);
        const int h = (int)(factor * (double)H), w = (int)(factor * (double)W);
        const int top = aug_position(s, lane, H, h), left = aug_position(s, lane, W, w);
        y0 -= (double)top; y1 -= (double)top; x0 -= (double)left; x1 -= (double)left;      // CropPad: labels -= (top, left); no filter, no clip
        g[0] = 1; g[1] = top; g[2] = left; g[3] = h; g[4] = w;
        H = h; W = w;
    }
    g[8] = H; g[9] = W;

    // ---- SSDRandomCrop: RandomPatchInf -- rounds until a valid patch or the "leave it" draw -------------------------------------------
    for (int round = 0; round < p.max_rounds; ++round) {
        if (mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.crop_prob)) break;                    // unaltered
        const double u = mt_double(s, lane);                                               // BoundGenerator: np.random.choice(n, p=weights)
        int bi = 0;
        while (bi < p.n_bounds - 1 && !(u < p.cdf[bi])) ++bi;                               // searchsorted(cdf, u, side='right')
        const double lower = p.lower[bi], upper = p.upper[bi];
        bool found = false;
        for (int t = 0; t < p.n_trials && !found; ++t) {
            const int h = (int)(mt_uniform(s, lane, p.crop_min, p.crop_max) * (double)H);
            const int w = (int)(mt_uniform(s, lane, p.crop_min, p.crop_max) * (double)W);
            const int top = aug_position(s, lane, H, h), left = aug_position(s, lane, W, w);
            const double ar = (double)w / (double)h;
            if (!(p.ar_min <= ar && ar <= p.ar_max)) continue;
            // ImageValidator('iou', bounds, n_boxes_min = 1, border 'half'): iou(patch, box shifted into the patch's frame) in (lower, upper]
            PxBox<double> im, bb;
            im.x0 = 0.0; im.y0 = 0.0; im.x1 = (double)w; im.y1 = (double)h;
            im.area = box_area<double>(im.x0, im.y0, im.x1, im.y1, 0.0);
            bb.x0 = x0 - (double)left; bb.y0 = y0 - (double)top; bb.x1 = x1 - (double)left; bb.y1 = y1 - (double)top;
            bb.area = box_area<double>(bb.x0, bb.y0, bb.x1, bb.y1, 0.0);
            const double v = iou_px<double>(im, bb);
            if (__ballot(alive && v > lower && v <= upper) == 0ull) continue;
            // the cut: CropPad(clip_boxes=True, box_filter = centre point inside the patch)
            x0 = bb.x0; y0 = bb.y0; x1 = bb.x1; y1 = bb.y1;
            const double cy = (y0 + y1) / 2.0, cx = (x0 + x1) / 2.0;
            alive = alive && cy >= 0.0 && cy <= (double)h - 1.0 && cx >= 0.0 && cx <= (double)w - 1.0;
            const double ymax = (double)(h - 1), xmax = (double)(w - 1);
            y0 = y0 < 0.0 ? 0.0 : (y0 > ymax ? ymax : y0); y1 = y1 < 0.0 ? 0.0 : (y1 > ymax ? ymax : y1);
            x0 = x0 < 0.0 ? 0.0 : (x0 > xmax ? xmax : x0); x1 = x1 < 0.0 ? 0.0 : (x1 > xmax ? xmax : x1);
            g[5] = 1; g[6] = top; g[7] = left; g[8] = h; g[9] = w;
            H = h; W = w;
            found = true;
        }
        if (found) break;
    }

    // ---- RandomFlip('horizontal', prob) ----------------------------------------------------------------------------------------------
    if (!(mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.flip_prob))) {
        const double nx0 = (double)W - x1, nx1 = (double)W - x0;
        x0 = nx0; x1 = nx1;
        g[10] = 1;
    }

    // ---- ResizeRandomInterp: mode = np.random.choice(modes); Resize's label arithmetic + the degenerate-box filter -----------------------
    g[11] = p.modes[(int)mt_randint(s, lane, 0, p.n_modes)];
    {
        const double sy = (double)p.out_h / (double)H, sx = (double)p.out_w / (double)W;
        y0 = __builtin_rint(y0 * sy); y1 = __builtin_rint(y1 * sy);
        x0 = __builtin_rint(x0 * sx); x1 = __builtin_rint(x1 * sx);
        alive = alive && x1 > x0 && y1 > y0;
    }

    const u64 keep = __ballot(alive);
    if (alive) {
        const int pos = __popcll(keep & lanemask_lt());
        double* r = lab_out + ((size_t)b * AUG_MAXG + pos) * 5;
        r[0] = cls; r[1] = x0; r[2] = y0; r[3] = x1; r[4] = y1;
    }
    if (lane == 0) {
        n_out[b] = __popcll(keep);
        for (int i = 0; i < 12; ++i) geo[(size_t)b * 12 + i] = g[i];
    }
}

// one wave per image, every image on its OWN generator state (augment_batch(seeds=...), round 5)
__global__ __launch_bounds__(64) void ssd_augment_decide_kernel(AugParams p, const u32* __restrict__ mt_in, const double* __restrict__ lab_in,
                                                                const int* __restrict__ n_in, int* __restrict__ geo,
                                                                double* __restrict__ lab_out, int* __restrict__ n_out,
                                                                u32* __restrict__ mt_out) {
    __shared__ u32 key[624];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    for (int i = lane; i < 624; i += 64) key[i] = mt_in[(size_t)b * 625 + i];
    Mt s;
    s.key = key;
    s.pos = (int)mt_in[(size_t)b * 625 + 624];
    s.base = -1; s.win = 0u;
    __syncthreads();
    aug_decide_image(p, s, lane, b, p.H, p.W, lab_in, n_in, geo, lab_out, n_out);
    if (lane == 0) mt_out[(size_t)b * 625 + 624] = (u32)s.pos;
    __syncthreads();
    for (int i = lane; i < 624; i += 64) mt_out[(size_t)b * 625 + i] = key[i];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Round 6: the reference's OWN contract -- ONE generator for the whole batch.  Its generator loop calls the chain image after image on the
// global np.random stream (object_detection_2d_data_generator.py:1050-1089 -> data_augmentation_chain_original_ssd.py:208-280), so the
// draws of image i + 1 start where image i's ended: inherently serial, and cheap (a few dozen draws per image).  ONE wave walks the batch
// in order on that one stream and takes EVERY decision, the photometric ones included (SSDPhotometricDistortions :146-208: which of the
// two sequences, and per op "does it fire" + its parameter), writing them as the per-image programs ssdhip_image_program runs; the
// geometric half is aug_decide_image.  Out: the programs, the geometry, the labels and the generator state behind the LAST image, which
// the host writes back into np.random -- the stream continues exactly as if the reference's loop had run.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct AugPhoto {                                         // RandomBrightness / Contrast / Saturation / Hue: prob, uniform(lo, hi); swap: prob 0
    double prob[4], lo[4], hi[4], swap_prob;
};
constexpr int AUG_PROG = 16;
// The size of image b: the batch's (uniform) or the image's own from the ragged table [B][4] int64 = byte offset, H, W, C.
struct UniformHW {
    int H, W;
    __device__ __forceinline__ int h(int) const { return H; }
    __device__ __forceinline__ int w(int) const { return W; }
};
struct RaggedHW {
    const long long* table;
    __device__ __forceinline__ int h(int b) const { return (int)table[(size_t)b * 4 + 1]; }
    __device__ __forceinline__ int w(int b) const { return (int)table[(size_t)b * 4 + 2]; }
};                              // steps of a program (include/ssdhip.h: SSDHIP_IMG_PROG)
enum { OP_END = 0, OP_TO_F32 = 1, OP_TO_U8 = 2, OP_BRIGHTNESS = 3, OP_CONTRAST = 4, OP_SATURATION = 5, OP_HUE = 6, OP_RGB2HSV = 7, OP_HSV2RGB = 8 };

// The photometric draws of one image as its program for ssdhip_image_program (SSDPhotometricDistortions.draw and
// DataAugmentationConstantInputSize._draw): `if np.random.choice(2)` picks the sequence, every random op -- brightness, contrast,
// saturation, hue = entries 0 .. 3 of prob / lo / hi -- draws uniform(0, 1) and, when it fires (>= 1 - prob), its parameter
// uniform(lo, hi).  swap_draw: a RandomChannelSwap(prob = 0.0) ends the sequence -- its uniform(0, 1) >= 1.0 never holds, the draw is
// consumed.  choose_sequence = false: a chain with ONE fixed list of transforms (DataAugmentationVariableInputSize) -- no
// `np.random.choice(2)` draw, the order is sequence 1's.  Returns whether sequence 1 (contrast before the HSV part) runs.
__device__ __forceinline__ bool aug_photo_program(Mt& s, const int lane, const double* prob, const double* lo, const double* hi,
                                                  const bool choose_sequence, const bool swap_draw, const int b,
                                                  int* __restrict__ prog_ops, double* __restrict__ prog_args) {
    int ops[AUG_PROG];
    double args[AUG_PROG];
    int k = 0;
    auto push = [&](int op, double a) { ops[k] = op; args[k] = a; ++k; };
    auto maybe = [&](int which, int op) {                // RandomX.draw(): the firing draw, then uniform(lower, upper)
        if (mt_uniform(s, lane, 0.0, 1.0) >= (1.0 - prob[which])) push(op, mt_uniform(s, lane, lo[which], hi[which]));
    };
    const bool contrast_first = choose_sequence ? mt_randint(s, lane, 0, 2) != 0 : true;
    push(OP_TO_F32, 0.0);
    maybe(0, OP_BRIGHTNESS);
    if (contrast_first) maybe(1, OP_CONTRAST);
    push(OP_TO_U8, 0.0); push(OP_RGB2HSV, 0.0); push(OP_TO_F32, 0.0);
    maybe(2, OP_SATURATION);
    maybe(3, OP_HUE);
    push(OP_TO_U8, 0.0); push(OP_HSV2RGB, 0.0);
    if (!contrast_first) { push(OP_TO_F32, 0.0); maybe(1, OP_CONTRAST); push(OP_TO_U8, 0.0); }
    if (swap_draw) (void)mt_uniform(s, lane, 0.0, 1.0);
    for (; k < AUG_PROG; ) push(OP_END, 0.0);
    if (lane == 0)
        for (int i = 0; i < AUG_PROG; ++i) { prog_ops[(size_t)b * AUG_PROG + i] = ops[i]; prog_args[(size_t)b * AUG_PROG + i] = args[i]; }
    return contrast_first;
}

template <class HW>
__global__ __launch_bounds__(64) void ssd_augment_stream_kernel(AugParams p, AugPhoto ph, HW hw, int B, const u32* __restrict__ mt_in,
                                                                const double* __restrict__ lab_in, const int* __restrict__ n_in,
                                                                int* __restrict__ prog_ops, double* __restrict__ prog_args,
                                                                int* __restrict__ geo, double* __restrict__ lab_out, int* __restrict__ n_out,
                                                                u32* __restrict__ mt_out) {
    __shared__ u32 key[624];
    const int lane = (int)threadIdx.x;
    for (int i = lane; i < 624; i += 64) key[i] = mt_in[i];
    Mt s;
    s.key = key;
    s.pos = (int)mt_in[624];
    s.base = -1; s.win = 0u;
    __syncthreads();
    for (int b = 0; b < B; ++b) {
        // ---- SSDPhotometricDistortions.__call__; RandomChannelSwap(prob 0) draws and never fires ---------------------------------------
        (void)aug_photo_program(s, lane, ph.prob, ph.lo, ph.hi, true, true, b, prog_ops, prog_args);
        // ---- the geometric half on the same stream ------------------------------------------------------------------------------------
        aug_decide_image(p, s, lane, b, hw.h(b), hw.w(b), lab_in, n_in, geo, lab_out, n_out);
    }
    if (lane == 0) mt_out[624] = (u32)s.pos;
    __syncthreads();
    for (int i = lane; i < 624; i += 64) mt_out[i] = key[i];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Round 6: the gather launch's PLANS with cv2.resize's own 8-bit arithmetic (ssdhip_image_resize_gather_cv_u8), built on the device from
// the decisions: per image the dispatch of cv::resize (copy / nearest / fixed-point linear, cubic, Lanczos-4 / area-mode bilinear /
// ResizeArea / ResizeAreaFast) and per axis the tap indices + table values of data_generator/_image_ops.py resize_plan -- the same
// float32 / float64 operations in the same order (this file is compiled without contraction), Lanczos' sine and cosine by the same
// fixed Horner chain -- composed with the recorded geometry (resize <- flip <- crop window <- expansion canvas; -1 = a canvas pixel,
// filled with the background colour).
// ---------------------------------------------------------------------------------------------------------------------------------------
enum { PK_NEAREST = 0, PK_LINEAR = 1, PK_KERNEL = 2, PK_AREA = 3, PK_AREA_FAST = 4, PK_AREA_FAST2 = 5, PK_COPY = 6 };
__device__ const double AUG_SIN_C[12] = {1.0, 0.16666666666666666, 0.008333333333333333, 0.0001984126984126984, 2.7557319223985893e-06, 2.505210838544172e-08, 1.6059043836821613e-10, 7.647163731819816e-13, 2.8114572543455206e-15, 8.22063524662433e-18, 1.9572941063391263e-20, 3.8681701706306835e-23};       // 1 / (2 k + 1)!
__device__ const double AUG_COS_C[12] = {1.0, 0.5, 0.041666666666666664, 0.001388888888888889, 2.48015873015873e-05, 2.755731922398589e-07, 2.08767569878681e-09, 1.1470745597729725e-11, 4.779477332387385e-14, 1.5619206968586225e-16, 4.110317623312165e-19, 8.896791392450574e-22};       // 1 / (2 k)!

__device__ __forceinline__ void aug_sincos_near_minus_pi(double y, double& sn, double& cs) {   // _image_ops.sincos_near_minus_pi
    const double t = y + 3.1415926535897932384626433832795;
    const double t2 = t * t;
    double s = AUG_SIN_C[11];
    for (int k = 10; k >= 0; --k) s = AUG_SIN_C[k] - s * t2;
    double c = AUG_COS_C[11];
    for (int k = 10; k >= 0; --k) c = AUG_COS_C[k] - c * t2;
    sn = -(s * t);
    cs = -c;
}
__device__ __forceinline__ double aug_to_short(float coef) {                  // saturate_cast<short>(coef * 2048): nearest-even, clamped
    const double r = __builtin_rint((double)(coef * 2048.f));
    return r < -32768.0 ? -32768.0 : (r > 32767.0 ? 32767.0 : r);
}

struct AugPlan { int kind, area, tx, ty, interp, area_mode; };
__device__ __forceinline__ AugPlan aug_plan_of(int Hc, int Wc, int out_h, int out_w, int interp, int n_taps) {
    AugPlan q;
    q.area = 1; q.tx = 1; q.ty = 1; q.interp = interp; q.area_mode = 0;
    if (Hc == out_h && Wc == out_w) { q.kind = PK_COPY; return q; }
    if (interp == 0) { q.kind = PK_NEAREST; return q; }
    const double scale_x = 1.0 / ((double)out_w / (double)Wc), scale_y = 1.0 / ((double)out_h / (double)Hc);
    const int isx = (int)__builtin_rint(scale_x), isy = (int)__builtin_rint(scale_y);
    const double eps = 2.220446049250313e-16;
    const bool fast = fabs(scale_x - (double)isx) < eps && fabs(scale_y - (double)isy) < eps;
    if (interp == 1 && fast && isx == 2 && isy == 2) interp = 3;
    if (interp == 3 && scale_x >= 1.0 && scale_y >= 1.0) {
        if (fast) { q.kind = (isx == 2 && isy == 2) ? PK_AREA_FAST2 : PK_AREA_FAST; q.area = isx * isy; q.tx = isx; q.ty = isy; }
        else {
            q.kind = PK_AREA;
            const int bx = (int)ceil(scale_x) + 2, by = (int)ceil(scale_y) + 2;
            q.tx = bx < n_taps ? bx : n_taps; q.ty = by < n_taps ? by : n_taps;
        }
        q.interp = 3;
        return q;
    }
    q.interp = interp;
    q.area_mode = interp == 3;
    if (interp == 1 || interp == 3) { q.kind = PK_LINEAR; q.tx = q.ty = 2; }
    else { q.kind = PK_KERNEL; q.tx = q.ty = interp == 2 ? 4 : 8; }
    return q;
}

// The taps of destination position i of one axis (0 = columns, 1 = rows) of plan q: indices into the n_src positions of the image in front
// of the resize and the table values, idx / w [64]; returns how many.
__device__ __forceinline__ int aug_axis_taps(const AugPlan& q, const int axis, const int i, const int n_src, const int n_dst, int* idx,
                                             double* w) {
    const double inv = (double)n_dst / (double)n_src, scale = 1.0 / inv;
    int T = 1;
    if (q.kind == PK_COPY) { idx[0] = i; w[0] = 1.0; }
    else if (q.kind == PK_NEAREST) {
        const double f = floor((double)i * scale);
        idx[0] = (int)(f < (double)(n_src - 1) ? f : (double)(n_src - 1));
        w[0] = 1.0;
    } else if (q.kind == PK_AREA_FAST || q.kind == PK_AREA_FAST2) {
        const int is = axis == 0 ? q.tx : q.ty;
        T = is > 64 ? 64 : is;
        for (int t = 0; t < T; ++t) { idx[t] = i * is + t; w[t] = 1.0; }
    } else if (q.kind == PK_AREA) {                                         // computeResizeAreaTab, the entries of destination i
        const double f1 = (double)i * scale, f2 = f1 + scale;
        const double room = (double)n_src - f1;
        const double cell = scale < room ? scale : room;
        long long s2 = (long long)floor(f2), s1 = (long long)ceil(f1);
        s2 = s2 < n_src - 1 ? s2 : n_src - 1;
        s1 = s1 < s2 ? s1 : s2;
        T = 0;
        if ((double)s1 - f1 > 1e-3) { idx[T] = (int)(s1 - 1); w[T] = (double)(float)(((double)s1 - f1) / cell); ++T; }
        for (long long sx = s1; sx < s2 && T < 63; ++sx) { idx[T] = (int)sx; w[T] = (double)(float)(1.0 / cell); ++T; }
        if (f2 - (double)s2 > 1e-3) {
            double m = f2 - (double)s2;
            m = m < 1.0 ? m : 1.0;
            m = m < cell ? m : cell;
            idx[T] = (int)s2; w[T] = (double)(float)(m / cell); ++T;
        }
        if (T == 0) { idx[0] = 0; w[0] = 0.0; T = 1; }
        for (int t = 0; t < T; ++t) idx[t] = idx[t] < 0 ? 0 : (idx[t] > n_src - 1 ? n_src - 1 : idx[t]);
    } else {
        long long sx;
        float fx;
        if (q.area_mode) {
            sx = (long long)floor((double)i * scale);
            fx = (float)(((double)i + 1.0) - ((double)sx + 1.0) * inv);
            fx = fx <= 0.f ? 0.f : fx - floorf(fx);
        } else {
            fx = (float)(((double)i + 0.5) * scale - 0.5);
            const float fl = floorf(fx);
            sx = (long long)fl;
            fx = fx - fl;
        }
        int off0;
        float co[8];
        if (q.kind == PK_LINEAR) {
            if (axis == 0) {                                                // only the x loop resets the pair at the borders
                if (sx < 0) { sx = 0; fx = 0.f; }
                else if (sx >= n_src - 1) { sx = n_src - 1; fx = 0.f; }
            }
            off0 = 0; T = 2;
            co[0] = 1.f - fx; co[1] = fx;
        } else if (q.interp == 2) {                                         // interpolateCubic, A = -0.75, float32 operation by operation
            off0 = -1; T = 4;
            const float A = -0.75f, u = fx + 1.f, v = 1.f - fx;
            co[0] = ((A * u - 5.f * A) * u + 8.f * A) * u - 4.f * A;
            co[1] = ((A + 2.f) * fx - (A + 3.f)) * fx * fx + 1.f;
            co[2] = ((A + 2.f) * v - (A + 3.f)) * v * v + 1.f;
            co[3] = 1.f - co[0] - co[1] - co[2];
        } else {                                                            // interpolateLanczos4
            off0 = -3; T = 8;
            if (fx < 1.1920928955078125e-07f) {
                for (int t = 0; t < 8; ++t) co[t] = 0.f;
                co[3] = 1.f;
            } else {
                const double r = 0.70710678118654752440084436210485;
                const double cs[8][2] = {{1, 0}, {-r, -r}, {0, 1}, {r, -r}, {-1, 0}, {r, r}, {0, -1}, {-r, r}};
                const float x3 = fx + 3.f;
                double s0, c0;
                aug_sincos_near_minus_pi(-((double)x3) * 3.1415926535897932384626433832795 * 0.25, s0, c0);
                float total = 0.f;
                for (int t = 0; t < 8; ++t) {
                    const double y = -((double)(x3 - (float)t)) * 3.1415926535897932384626433832795 * 0.25;
                    co[t] = (float)((cs[t][0] * s0 + cs[t][1] * c0) / (y * y));
                }
                for (int t = 0; t < 8; ++t) total = total + co[t];
                total = 1.f / total;
                for (int t = 0; t < 8; ++t) co[t] = co[t] * total;
            }
        }
        for (int t = 0; t < T; ++t) {
            const long long c = sx + off0 + t;
            idx[t] = (int)(c < 0 ? 0 : (c > n_src - 1 ? n_src - 1 : c));
            w[t] = aug_to_short(co[t]);
        }
    }
    return T;
}

// grid (blocks over positions, 2 axes, B); axis 0 = columns (x), 1 = rows (y); plan [B][4] = kind, area, taps per column, taps per row
template <class HW>
__global__ __launch_bounds__(128) void aug_plan_kernel(const int* __restrict__ geo, HW hw, int out_h, int out_w, int n_taps,
                                                       int* __restrict__ plan, int* __restrict__ ix, double* __restrict__ wx,
                                                       int* __restrict__ iy, double* __restrict__ wy) {
    const int b = (int)blockIdx.z, axis = (int)blockIdx.y;
    const int n_dst = axis == 0 ? out_w : out_h;
    const int i = (int)blockIdx.x * 128 + (int)threadIdx.x;
    const int* g = geo + (size_t)b * 12;
    const int H = hw.h(b), W = hw.w(b);
    const int Hc = g[8], Wc = g[9];
    const AugPlan q = aug_plan_of(Hc, Wc, out_h, out_w, g[11], n_taps);
    if (axis == 0 && i == 0) { plan[b * 4] = q.kind; plan[b * 4 + 1] = q.area; plan[b * 4 + 2] = q.tx; plan[b * 4 + 3] = q.ty; }
    if (i >= n_dst) return;
    const int n_src = axis == 0 ? Wc : Hc;
    int idx[64];
    double w[64];
    const int T = aug_axis_taps(q, axis, i, n_src, n_dst, idx, w);
    // the recorded geometry: position j of the final (pre-resize) image <- flip <- crop window <- expansion canvas <- the image
    int* oi = (axis == 0 ? ix : iy) + ((size_t)b * n_dst + i) * n_taps;
    double* ow = (axis == 0 ? wx : wy) + ((size_t)b * n_dst + i) * n_taps;
    for (int t = 0; t < n_taps; ++t) {
        int j = idx[t < T ? t : T - 1];
        if (axis == 0 && g[10]) j = Wc - 1 - j;                                   // RandomFlip('horizontal')
        if (g[5]) j += axis == 0 ? g[7] : g[6];                                   // the crop window's corner on the canvas
        if (g[0]) {                                                               // the canvas: the image sits at (-top, -left)
            j += axis == 0 ? g[2] : g[1];
            if (j < 0 || j >= (axis == 0 ? W : H)) j = -1;
        }
        oi[t] = j;
        ow[t] = t < T ? w[t] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// DataAugmentationConstantInputSize (data_generator/data_augmentation_chain_constant_input_size.py), the chain ssd7_training.ipynb
// trains with: per image `np.random.choice(2)` picks the sequence, the photometric draws follow in that sequence's order (`_draw`), then
// RandomTranslate / RandomScale / RandomFlip of object_detection_2d_geometric_ops.py run in the sequence's order -- their firing draws,
// their trial loops (ImageValidator on the candidate labels, the first valid trial ends the loop and the draws), and Translate's /
// Scale's / Flip's label arithmetic (shift or matrix + rint, BoxFilter, clip).  The host ran this per image with one validator / box-filter
// launch and download per trial (10.1 ms for a batch of 32 whose two pixel kernels take a fraction of that); here a wave does it on the
// image's MT19937 stream, lane = ground truth box.  The pixels stay where they were: the programs go to ssdhip_image_program, the
// geometry rows to const_plan_kernel below and from there to ssdhip_image_warp_affine_u8.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct ConstAugParams {
    int H, W;
    double ph_prob[4], ph_lo[4], ph_hi[4];                // RandomBrightness, RandomContrast, RandomSaturation, RandomHue
    double tr_prob, dy_lo, dy_hi, dx_lo, dx_hi;           // RandomTranslate
    double zin_prob, zin_lo, zin_hi;                      // RandomScale of sequence 1 (zoom in)
    double zout_prob, zout_lo, zout_hi;                   // RandomScale of sequence 2 (zoom out)
    double flip_prob;
    int n_trials, clip, n_min;                            // max(1, n_trials_max), clip_boxes, ImageValidator's n_boxes_min
    double val_lo, val_hi;                                // ImageValidator's bounds
    double flt_lo, flt_hi, min_area;                      // BoxFilter's overlap bounds and min_area
};
constexpr int CAUG_GEO = 8;                               // geometry row: sequence, translated?, dx, dy, scaled?, factor, flipped?, zoom first?

// BoxFilter's 'area' criterion with border_pixels 'half' (d = 0), as box_filter_kernel (csrc/ssdhip_boxes.hip) evaluates it: the box's
// area inside the image over its whole area within (lower, upper] -- [lower, upper] for a lower bound that is not 0.
__device__ __forceinline__ bool caug_area_ok(double xmin, double ymin, double xmax, double ymax, double H, double W, double lower,
                                             double upper) {
    const double d = 0.0;
    const double box_area_ = ((xmax - xmin) + d) * ((ymax - ymin) + d);
    const double cy0 = np_minimum<double>(np_maximum<double>(ymin, 0.0), H - 1.0), cy1 = np_minimum<double>(np_maximum<double>(ymax, 0.0), H - 1.0);
    const double cx0 = np_minimum<double>(np_maximum<double>(xmin, 0.0), W - 1.0), cx1 = np_minimum<double>(np_maximum<double>(xmax, 0.0), W - 1.0);
    const double inter = ((cx1 - cx0) + d) * ((cy1 - cy0) + d);
    const bool lo = lower == 0.0 ? (inter > lower * box_area_) : (inter >= lower * box_area_);
    return lo && (inter <= upper * box_area_);
}
// the chain's BoxFilter (check_overlap 'area', check_min_area, check_degenerate), then the clip of Translate / Scale
__device__ __forceinline__ void caug_filter_clip(const ConstAugParams& p, bool& alive, double& x0, double& y0, double& x1, double& y1) {
    const double H = (double)p.H, W = (double)p.W;
    alive = alive && (x1 > x0) && (y1 > y0) && ((x1 - x0) * (y1 - y0) >= p.min_area) && caug_area_ok(x0, y0, x1, y1, H, W, p.flt_lo, p.flt_hi);
    if (p.clip) {
        y0 = np_minimum<double>(np_maximum<double>(y0, 0.0), H - 1.0); y1 = np_minimum<double>(np_maximum<double>(y1, 0.0), H - 1.0);
        x0 = np_minimum<double>(np_maximum<double>(x0, 0.0), W - 1.0); x1 = np_minimum<double>(np_maximum<double>(x1, 0.0), W - 1.0);
    }
}
// _image_ops.rotation_matrix_2d((W / 2, H / 2), 0, factor): the centre is a Point2f, the result float64
__device__ __forceinline__ void caug_matrix(double factor, int H, int W, double* m) {
    const double cx = (double)(float)((double)W / 2.0), cy = (double)(float)((double)H / 2.0);
    const double a = 1.0 * factor, b = 0.0 * factor;     // cos(0) scale, sin(0) scale
    m[0] = a; m[1] = b; m[2] = (1.0 - a) * cx - b * cy;
    m[3] = -b; m[4] = a; m[5] = b * cx + (1.0 - a) * cy;
}

// RandomTranslate.__call__ (:200-224) + Translate's label arithmetic (:154-172)
__device__ __forceinline__ void caug_translate(const ConstAugParams& p, Mt& s, const int lane, bool& alive, double& x0, double& y0,
                                               double& x1, double& y1, double* g) {
    if (!(mt_uniform(s, lane, 0.0, 1.0) >= (1.0 - p.tr_prob))) return;
    for (int t = 0; t < p.n_trials; ++t) {
        const double dy_abs = mt_uniform(s, lane, p.dy_lo, p.dy_hi);
        const double dx_abs = mt_uniform(s, lane, p.dx_lo, p.dx_hi);
        const double dy = mt_randint(s, lane, 0, 2) ? dy_abs : -dy_abs;       // np.random.choice([-dy_abs, dy_abs])
        const double dx = mt_randint(s, lane, 0, 2) ? dx_abs : -dx_abs;
        const double sy = __builtin_rint((double)p.H * dy), sx = __builtin_rint((double)p.W * dx);   // int(round(.)): ties to even
        const bool ok = alive && caug_area_ok(x0 + sx, y0 + sy, x1 + sx, y1 + sy, (double)p.H, (double)p.W, p.val_lo, p.val_hi);
        if (__popcll(__ballot(ok)) < p.n_min) continue;
        x0 += sx; x1 += sx; y0 += sy; y1 += sy;
        caug_filter_clip(p, alive, x0, y0, x1, y1);
        g[1] = 1.0; g[2] = sx; g[3] = sy;
        return;
    }
}
// RandomScale.__call__ (:282-304) + Scale's label arithmetic (:241-258): the corners through M as np.dot(M, [x, y, 1]) sums them
__device__ __forceinline__ void caug_scale(const ConstAugParams& p, Mt& s, const int lane, double prob, double lo, double hi, bool& alive,
                                           double& x0, double& y0, double& x1, double& y1, double* g) {
    if (!(mt_uniform(s, lane, 0.0, 1.0) >= (1.0 - prob))) return;
    for (int t = 0; t < p.n_trials; ++t) {
        const double factor = mt_uniform(s, lane, lo, hi);
        double m[6];
        caug_matrix(factor, p.H, p.W, m);
        const double nx0 = __builtin_rint((m[0] * x0 + m[1] * y0) + m[2] * 1.0), ny0 = __builtin_rint((m[3] * x0 + m[4] * y0) + m[5] * 1.0);
        const double nx1 = __builtin_rint((m[0] * x1 + m[1] * y1) + m[2] * 1.0), ny1 = __builtin_rint((m[3] * x1 + m[4] * y1) + m[5] * 1.0);
        const bool ok = alive && caug_area_ok(nx0, ny0, nx1, ny1, (double)p.H, (double)p.W, p.val_lo, p.val_hi);
        if (__popcll(__ballot(ok)) < p.n_min) continue;
        x0 = nx0; y0 = ny0; x1 = nx1; y1 = ny1;
        caug_filter_clip(p, alive, x0, y0, x1, y1);
        g[4] = 1.0; g[5] = factor;
        return;
    }
}

// ONE image of the chain by one wave on the generator state `s`: `_draw`, then the three geometric ops.
__device__ __forceinline__ void caug_decide_image(const ConstAugParams& p, Mt& s, const int lane, const int b,
                                                  const double* __restrict__ lab_in, const int* __restrict__ n_in,
                                                  int* __restrict__ prog_ops, double* __restrict__ prog_args, double* __restrict__ geo,
                                                  double* __restrict__ lab_out, int* __restrict__ n_out) {
    // ---- _draw: the sequence choice and the photometric draws in that sequence's order (this chain has no channel swap) ---------------
    const bool seq1 = aug_photo_program(s, lane, p.ph_prob, p.ph_lo, p.ph_hi, true, false, b, prog_ops, prog_args);

    // ---- the geometric ops on the same stream: translate, zoom in, flip | zoom out, translate, flip -----------------------------------
    const int n = n_in[b];
    bool alive = lane < n;
    double cls = 0.0, x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;
    if (alive) {
        const double* r = lab_in + ((size_t)b * AUG_MAXG + lane) * 5;
        cls = r[0]; x0 = r[1]; y0 = r[2]; x1 = r[3]; y1 = r[4];
    }
    double g[CAUG_GEO] = {seq1 ? 1.0 : 2.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, seq1 ? 0.0 : 1.0};
    if (seq1) {
        caug_translate(p, s, lane, alive, x0, y0, x1, y1, g);
        caug_scale(p, s, lane, p.zin_prob, p.zin_lo, p.zin_hi, alive, x0, y0, x1, y1, g);
    } else {
        caug_scale(p, s, lane, p.zout_prob, p.zout_lo, p.zout_hi, alive, x0, y0, x1, y1, g);
        caug_translate(p, s, lane, alive, x0, y0, x1, y1, g);
    }
    if (!(mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.flip_prob))) {                           // RandomFlip('horizontal') :121-125, Flip :99-105
        const double nx0 = (double)p.W - x1, nx1 = (double)p.W - x0;
        x0 = nx0; x1 = nx1;
        g[6] = 1.0;
    }

    const u64 keep = __ballot(alive);
    if (alive) {
        const int pos = __popcll(keep & lanemask_lt());
        double* r = lab_out + ((size_t)b * AUG_MAXG + pos) * 5;
        r[0] = cls; r[1] = x0; r[2] = y0; r[3] = x1; r[4] = y1;
    }
    if (lane == 0) {
        n_out[b] = __popcll(keep);
        for (int i = 0; i < CAUG_GEO; ++i) geo[(size_t)b * CAUG_GEO + i] = g[i];
    }
}

// STREAM = false: one wave per image, image b on its own state (mt [B][625]); true: one wave walks the B images in order on one state
template <bool STREAM>
__global__ __launch_bounds__(64) void const_augment_decide_kernel(ConstAugParams p, int B, const u32* __restrict__ mt_in,
                                                                  const double* __restrict__ lab_in, const int* __restrict__ n_in,
                                                                  int* __restrict__ prog_ops, double* __restrict__ prog_args,
                                                                  double* __restrict__ geo, double* __restrict__ lab_out,
                                                                  int* __restrict__ n_out, u32* __restrict__ mt_out) {
    __shared__ u32 key[624];
    const int lane = (int)threadIdx.x;
    const size_t at = STREAM ? 0 : (size_t)blockIdx.x * 625;
    for (int i = lane; i < 624; i += 64) key[i] = mt_in[at + i];
    Mt s;
    s.key = key;
    s.pos = (int)mt_in[at + 624];
    s.base = -1; s.win = 0u;
    __syncthreads();
    if (STREAM) {
        for (int b = 0; b < B; ++b) caug_decide_image(p, s, lane, b, lab_in, n_in, prog_ops, prog_args, geo, lab_out, n_out);
    } else {
        caug_decide_image(p, s, lane, (int)blockIdx.x, lab_in, n_in, prog_ops, prog_args, geo, lab_out, n_out);
    }
    if (lane == 0) mt_out[at + 624] = (u32)s.pos;
    __syncthreads();
    for (int i = lane; i < 624; i += 64) mt_out[at + i] = key[i];
}

// The geometry rows -> what ssdhip_image_warp_affine_u8 takes, by _image_ops.WarpImage's composition rules (a whole-pixel translation
// before the zoom, or without one, is `pre`; one after it is `post`; a zoom by exactly 1 is a translation by (0, 0)) and the float64
// arithmetic of _image_ops.invert_affine / warp_tables.  grid (blocks over positions, 2 axes, B); axis 0 = columns, 1 = rows.
__global__ __launch_bounds__(128) void const_plan_kernel(const double* __restrict__ geometry, int H, int W, int* __restrict__ geo,
                                                         int* __restrict__ xtab, int* __restrict__ ytab) {
    const int b = (int)blockIdx.z, axis = (int)blockIdx.y;
    const int i = (int)blockIdx.x * 128 + (int)threadIdx.x;
    const double* g = geometry + (size_t)b * CAUG_GEO;
    const bool translated = g[1] != 0.0, scaled = g[4] != 0.0 && g[5] != 1.0;
    if (axis == 0 && i == 0) {
        const bool post = translated && scaled && g[7] != 0.0;
        const int dx = translated ? (int)g[2] : 0, dy = translated ? (int)g[3] : 0;
        int* o = geo + (size_t)b * 5;
        o[0] = g[6] != 0.0 ? 1 : 0;
        o[1] = post ? 0 : dx; o[2] = post ? 0 : dy;
        o[3] = post ? dx : 0; o[4] = post ? dy : 0;
    }
    double m[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (scaled) caug_matrix(g[5], H, W, m);
    double d = m[0] * m[4] - m[1] * m[3];                                     // invert_affine
    d = d != 0.0 ? 1.0 / d : 0.0;
    const double a11 = m[4] * d, a22 = m[0] * d;
    m[0] = a11; m[1] = m[1] * -d; m[3] = m[3] * -d; m[4] = a22;
    const double b1 = -m[0] * m[2] - m[1] * m[5];
    const double b2 = -m[3] * m[2] - m[4] * m[5];
    m[2] = b1; m[5] = b2;
    const double v = (double)i;                                               // warp_tables
    if (axis == 0 && i < W) {
        int* o = xtab + ((size_t)b * W + i) * 2;
        o[0] = (int)__builtin_rint(m[0] * v * 1024.0);
        o[1] = (int)__builtin_rint(m[3] * v * 1024.0);
    } else if (axis == 1 && i < H) {
        int* o = ytab + ((size_t)b * H + i) * 2;
        o[0] = (int)(__builtin_rint((m[1] * v + m[2]) * 1024.0) + 16.0);
        o[1] = (int)(__builtin_rint((m[4] * v + m[5]) * 1024.0) + 16.0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// DataAugmentationVariableInputSize (data_generator/data_augmentation_chain_variable_input_size.py), the chain for a dataset of images of
// different sizes: ONE list of transforms -- the photometric ops in sequence 1's order (no sequence draw, no channel swap), then
// RandomPatch(prob, can_fail = False) over PatchCoordinateGenerator(must_match = 'w_ar') with ONE overlap criterion ('area' | 'iou' |
// 'center_point') behind both its ImageValidator and its BoxFilter, RandomFlip('horizontal') and Resize with a (min_area, degenerate) box
// filter.  The host ran a validator launch + download per patch search and a box-filter launch + download per cut and per resize; here a
// wave does it on the image's MT19937 stream, lane = ground truth box.  The patch goes into the FIRST window slot of the 12-int geometry
// record aug_plan_kernel reads: unlike SSDExpand's canvas it may CUT the image on either axis, which that kernel's `j + top / left outside
// [0, H) / [0, W) -> -1` covers as it stands.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct VarAugParams {
    double ph_prob[4], ph_lo[4], ph_hi[4];                // RandomBrightness, RandomContrast, RandomSaturation, RandomHue
    double patch_prob, scale_lo, scale_hi, ar_lo, ar_hi;  // RandomPatch(prob); PatchCoordinateGenerator: scales of the width, aspect ratios
    int n_trials, clip;                                   // max(1, n_trials_max), clip_boxes
    int criterion, n_min;                                 // SSDHIP_VAR_AUG_*; ImageValidator's n_boxes_min, 0 = 'all'
    double val_lo, val_hi, flt_lo, flt_hi;                // ImageValidator's bounds, the patch BoxFilter's overlap bounds
    double flip_prob;
    int out_h, out_w, interp;                             // Resize
    double min_area;                                      // the resize BoxFilter's min_area (degenerate boxes dropped too)
};

// BoxFilter's overlap test (border_pixels 'half') of a box against an H x W image, as box_filter_kernel (csrc/ssdhip_boxes.hip) has it
__device__ __forceinline__ bool vaug_overlap_ok(const int criterion, double x0, double y0, double x1, double y1, double H, double W,
                                                double lower, double upper) {
    if (criterion == SSDHIP_VAR_AUG_IOU) {
        PxBox<double> im, bb;
        im.x0 = 0.0; im.y0 = 0.0; im.x1 = W; im.y1 = H;
        im.area = box_area<double>(im.x0, im.y0, im.x1, im.y1, 0.0);
        bb.x0 = x0; bb.y0 = y0; bb.x1 = x1; bb.y1 = y1;
        bb.area = box_area<double>(x0, y0, x1, y1, 0.0);
        const double v = iou_px<double>(im, bb);
        return v > lower && v <= upper;
    }
    if (criterion == SSDHIP_VAR_AUG_AREA) return caug_area_ok(x0, y0, x1, y1, H, W, lower, upper);
    const double cy = (y0 + y1) / 2.0, cx = (x0 + x1) / 2.0;
    return cy >= 0.0 && cy <= H - 1.0 && cx >= 0.0 && cx <= W - 1.0;
}

// The labels of image b, one box per lane: returns the clamped count, `alive` = this lane holds a box.
__device__ __forceinline__ int vaug_load_labels(const int lane, const int b, const double* __restrict__ lab_in, const int* __restrict__ n_in,
                                                bool& alive, double& cls, double& x0, double& y0, double& x1, double& y1) {
    int n = n_in[b];
    n = n < 0 ? 0 : (n > AUG_MAXG ? AUG_MAXG : n);
    alive = lane < n;
    cls = 0.0; x0 = 0.0; y0 = 0.0; x1 = 0.0; y1 = 0.0;
    if (alive) {
        const double* r = lab_in + ((size_t)b * AUG_MAXG + lane) * 5;
        cls = r[0]; x0 = r[1]; y0 = r[2]; x1 = r[3]; y1 = r[4];
    }
    return n;
}

// RandomPatch on an H x W image: the firing draw, then up to n_trials patches; the first one the validator accepts is cut (CropPad: shift,
// box filter, clip) and becomes the image -- win = (top, left, height, width), H and W the patch's.  Returns whether a patch was cut.
__device__ __forceinline__ bool vaug_random_patch(const VarAugParams& p, Mt& s, const int lane, const int n, bool& alive, double& x0, double& y0,
                                                  double& x1, double& y1, int& H, int& W, int* win) {
    if (!(mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.patch_prob))) {
        for (int t = 0; t < p.n_trials; ++t) {
            const int w = (int)(mt_uniform(s, lane, p.scale_lo, p.scale_hi) * (double)W);
            const double ar = mt_uniform(s, lane, p.ar_lo, p.ar_hi);
            const int h = (int)((double)w / ar);
            const int top = aug_position(s, lane, H, h), left = aug_position(s, lane, W, w);
            const double sx0 = x0 - (double)left, sy0 = y0 - (double)top, sx1 = x1 - (double)left, sy1 = y1 - (double)top;
            const bool ok = alive && vaug_overlap_ok(p.criterion, sx0, sy0, sx1, sy1, (double)h, (double)w, p.val_lo, p.val_hi);
            const int n_ok = __popcll(__ballot(ok));
            if (p.n_min > 0 ? n_ok < p.n_min : n_ok != n) continue;
            x0 = sx0; y0 = sy0; x1 = sx1; y1 = sy1;
            alive = alive && vaug_overlap_ok(p.criterion, x0, y0, x1, y1, (double)h, (double)w, p.flt_lo, p.flt_hi);
            if (p.clip) {
                const double ymax = (double)h - 1.0, xmax = (double)w - 1.0;
                y0 = np_minimum<double>(np_maximum<double>(y0, 0.0), ymax); y1 = np_minimum<double>(np_maximum<double>(y1, 0.0), ymax);
                x0 = np_minimum<double>(np_maximum<double>(x0, 0.0), xmax); x1 = np_minimum<double>(np_maximum<double>(x1, 0.0), xmax);
            }
            win[0] = top; win[1] = left; win[2] = h; win[3] = w;
            H = h; W = w;
            return true;
        }
    }
    return false;
}

// Resize: no draw; np.round(coordinate * (out / size)), then the (degenerate, min_area) box filter
__device__ __forceinline__ void vaug_resize_labels(const VarAugParams& p, const int H, const int W, bool& alive, double& x0, double& y0,
                                                   double& x1, double& y1) {
    const double sy = (double)p.out_h / (double)H, sx = (double)p.out_w / (double)W;
    y0 = __builtin_rint(y0 * sy); y1 = __builtin_rint(y1 * sy);
    x0 = __builtin_rint(x0 * sx); x1 = __builtin_rint(x1 * sx);
    alive = alive && x1 > x0 && y1 > y0 && ((x1 - x0) * (y1 - y0) >= p.min_area);
}

// The surviving boxes of image b, compacted in lane order, their count and the 12-int geometry record.
__device__ __forceinline__ void vaug_store(const int lane, const int b, const bool alive, double cls, double x0, double y0, double x1, double y1,
                                           const int* g, int* __restrict__ geo, double* __restrict__ lab_out, int* __restrict__ n_out) {
    const u64 keep = __ballot(alive);
    if (alive) {
        const int pos = __popcll(keep & lanemask_lt());
        double* r = lab_out + ((size_t)b * AUG_MAXG + pos) * 5;
        r[0] = cls; r[1] = x0; r[2] = y0; r[3] = x1; r[4] = y1;
    }
    if (lane == 0) {
        n_out[b] = __popcll(keep);
        for (int i = 0; i < 12; ++i) geo[(size_t)b * 12 + i] = g[i];
    }
}

// ONE image of the chain by one wave on the generator state `s`; (H0, W0): the image's size.
__device__ __forceinline__ void vaug_decide_image(const VarAugParams& p, Mt& s, const int lane, const int b, const int H0, const int W0,
                                                  const double* __restrict__ lab_in, const int* __restrict__ n_in,
                                                  int* __restrict__ prog_ops, double* __restrict__ prog_args, int* __restrict__ geo,
                                                  double* __restrict__ lab_out, int* __restrict__ n_out) {
    (void)aug_photo_program(s, lane, p.ph_prob, p.ph_lo, p.ph_hi, false, false, b, prog_ops, prog_args);

    bool alive;
    double cls, x0, y0, x1, y1;
    const int n = vaug_load_labels(lane, b, lab_in, n_in, alive, cls, x0, y0, x1, y1);
    int H = H0, W = W0;
    int g[12] = {0, 0, 0, H, W, 0, 0, 0, H, W, 0, p.interp};

    // ---- RandomPatch ---------------------------------------------------------------------------------------------------------------
    if (vaug_random_patch(p, s, lane, n, alive, x0, y0, x1, y1, H, W, g + 1)) g[0] = 1;
    g[8] = H; g[9] = W;

    // ---- RandomFlip('horizontal', prob) ----------------------------------------------------------------------------------------------
    if (!(mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.flip_prob))) {
        const double nx0 = (double)W - x1, nx1 = (double)W - x0;
        x0 = nx0; x1 = nx1;
        g[10] = 1;
    }

    vaug_resize_labels(p, H, W, alive, x0, y0, x1, y1);
    vaug_store(lane, b, alive, cls, x0, y0, x1, y1, g, geo, lab_out, n_out);
}

// STREAM = false: one wave per image, image b on its own state (mt [B][625]); true: one wave walks the B images in order on one state.
// HW: the images' one size, or each image's own from the ragged table.
template <bool STREAM, class HW>
__global__ __launch_bounds__(64) void var_augment_decide_kernel(VarAugParams p, HW hw, int B, const u32* __restrict__ mt_in,
                                                                const double* __restrict__ lab_in, const int* __restrict__ n_in,
                                                                int* __restrict__ prog_ops, double* __restrict__ prog_args,
                                                                int* __restrict__ geo, double* __restrict__ lab_out,
                                                                int* __restrict__ n_out, u32* __restrict__ mt_out) {
    __shared__ u32 key[624];
    const int lane = (int)threadIdx.x;
    const size_t at = STREAM ? 0 : (size_t)blockIdx.x * 625;
    for (int i = lane; i < 624; i += 64) key[i] = mt_in[at + i];
    Mt s;
    s.key = key;
    s.pos = (int)mt_in[at + 624];
    s.base = -1; s.win = 0u;
    __syncthreads();
    if (STREAM) {
        for (int b = 0; b < B; ++b)
            vaug_decide_image(p, s, lane, b, hw.h(b), hw.w(b), lab_in, n_in, prog_ops, prog_args, geo, lab_out, n_out);
    } else {
        const int b = (int)blockIdx.x;
        vaug_decide_image(p, s, lane, b, hw.h(b), hw.w(b), lab_in, n_in, prog_ops, prog_args, geo, lab_out, n_out);
    }
    if (lane == 0) mt_out[at + 624] = (u32)s.pos;
    __syncthreads();
    for (int i = lane; i < 624; i += 64) mt_out[at + i] = key[i];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// DataAugmentationSatellite (data_generator/data_augmentation_chain_satellite.py), the chain for images in bird's eye view: the variable
// chain's photometric draws, then RandomFlip('horizontal'), RandomFlip('vertical'), RandomRotate by 90 / 180 / 270 degrees, RandomPatch on
// the ROTATED image's height and width, and Resize.  The angle of a rotation is the one draw of the chain that comes from Python's
// `random`, not from NumPy: the host draws `random.choice(angles)` B times in advance from a copy of that generator and uploads the
// quarter turns (1 .. 3); a wave that walks the batch on one stream hands the k-th value to the k-th image that rotates, a wave on its own
// stream (one per image) takes value b.  Rotate's labels under the reference's adjusted matrix, for whole-number coordinates, are
//   90: (ymin, W - xmax, ymax, W - xmin)   180: (W - xmax, H - ymax, W - xmin, H - ymin)   270: (H - ymax, xmin, H - ymin, xmax)
// (H x W: the image in front of the rotation).  Geometry record, 12 ints: [0] patched? [1 .. 4] the patch's top, left, height, width on
// the rotated image (the first window slot of the other chains' record), [5] flipped horizontally? [6] vertically? [7] quarter turns,
// [8], [9] the size in front of the resize, [10] 0, [11] the interpolation mode.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct SatAugParams {
    VarAugParams v;                                       // v.flip_prob: the horizontal flip's
    double vflip_prob, rot_prob;
};

// ONE image by one wave; `turns`: the quarter turns this image takes IF it rotates.  Returns whether it rotated.
__device__ __forceinline__ bool saug_decide_image(const SatAugParams& p, Mt& s, const int lane, const int b, const int H0, const int W0,
                                                  int turns, const double* __restrict__ lab_in, const int* __restrict__ n_in,
                                                  int* __restrict__ prog_ops, double* __restrict__ prog_args, int* __restrict__ geo,
                                                  double* __restrict__ lab_out, int* __restrict__ n_out) {
    (void)aug_photo_program(s, lane, p.v.ph_prob, p.v.ph_lo, p.v.ph_hi, false, false, b, prog_ops, prog_args);

    bool alive;
    double cls, x0, y0, x1, y1;
    const int n = vaug_load_labels(lane, b, lab_in, n_in, alive, cls, x0, y0, x1, y1);
    int H = H0, W = W0;
    int g[12] = {0, 0, 0, H, W, 0, 0, 0, H, W, 0, p.v.interp};

    // ---- RandomFlip('horizontal', prob), RandomFlip('vertical', prob): `uniform < 1 - prob` leaves the image alone -----------------------
    if (!(mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.v.flip_prob))) {
        const double nx0 = (double)W - x1, nx1 = (double)W - x0;
        x0 = nx0; x1 = nx1;
        g[5] = 1;
    }
    if (!(mt_uniform(s, lane, 0.0, 1.0) < (1.0 - p.vflip_prob))) {
        const double ny0 = (double)H - y1, ny1 = (double)H - y0;
        y0 = ny0; y1 = ny1;
        g[6] = 1;
    }

    // ---- RandomRotate: `uniform >= 1 - prob` rotates, by the angle the host drew ------------------------------------------------------------
    const bool rotated = mt_uniform(s, lane, 0.0, 1.0) >= (1.0 - p.rot_prob);
    if (rotated) {
        turns = turns < 1 ? 1 : (turns > 3 ? 3 : turns);
        const double dH = (double)H, dW = (double)W;
        const double ax0 = x0, ay0 = y0, ax1 = x1, ay1 = y1;
        if (turns == 1) { x0 = ay0; y0 = dW - ax1; x1 = ay1; y1 = dW - ax0; }
        else if (turns == 2) { x0 = dW - ax1; y0 = dH - ay1; x1 = dW - ax0; y1 = dH - ay0; }
        else { x0 = dH - ay1; y0 = ax0; x1 = dH - ay0; y1 = ax1; }
        if (turns & 1) { const int t = H; H = W; W = t; }
        g[7] = turns;
    }

    // ---- RandomPatch on the rotated image, Resize ------------------------------------------------------------------------------------------
    g[3] = H; g[4] = W;
    if (vaug_random_patch(p.v, s, lane, n, alive, x0, y0, x1, y1, H, W, g + 1)) g[0] = 1;
    g[8] = H; g[9] = W;
    vaug_resize_labels(p.v, H, W, alive, x0, y0, x1, y1);
    vaug_store(lane, b, alive, cls, x0, y0, x1, y1, g, geo, lab_out, n_out);
    return rotated;
}

// STREAM / HW as var_augment_decide_kernel's; turns [B]: the quarter turns drawn on the host (see above).
template <bool STREAM, class HW>
__global__ __launch_bounds__(64) void sat_augment_decide_kernel(SatAugParams p, HW hw, int B, const int* __restrict__ turns,
                                                                const u32* __restrict__ mt_in, const double* __restrict__ lab_in,
                                                                const int* __restrict__ n_in, int* __restrict__ prog_ops,
                                                                double* __restrict__ prog_args, int* __restrict__ geo,
                                                                double* __restrict__ lab_out, int* __restrict__ n_out,
                                                                u32* __restrict__ mt_out) {
    __shared__ u32 key[624];
    const int lane = (int)threadIdx.x;
    const size_t at = STREAM ? 0 : (size_t)blockIdx.x * 625;
    for (int i = lane; i < 624; i += 64) key[i] = mt_in[at + i];
    Mt s;
    s.key = key;
    s.pos = (int)mt_in[at + 624];
    s.base = -1; s.win = 0u;
    __syncthreads();
    if (STREAM) {
        int k = 0;                                        // how many images have rotated so far (k <= b < B)
        for (int b = 0; b < B; ++b)
            if (saug_decide_image(p, s, lane, b, hw.h(b), hw.w(b), turns[k], lab_in, n_in, prog_ops, prog_args, geo, lab_out, n_out)) ++k;
    } else {
        const int b = (int)blockIdx.x;
        (void)saug_decide_image(p, s, lane, b, hw.h(b), hw.w(b), turns[b], lab_in, n_in, prog_ops, prog_args, geo, lab_out, n_out);
    }
    if (lane == 0) mt_out[at + 624] = (u32)s.pos;
    __syncthreads();
    for (int i = lane; i < 624; i += 64) mt_out[at + i] = key[i];
}

// The gather's plans for that record: resize taps <- patch window <- rotation <- vertical flip <- horizontal flip.  A rotated image is still
// two index maps: under the reference's matrices output pixel (row y, column x) of an H x W source reads source (column, row)
//   90: (W - y, x)     180: (W - x, H - y)     270: (y, H - x)
// so for 90 / 270 the ROW map (iy) addresses source columns and the column map (ix) source rows -- transposed [b] = 1 tells the gather to
// swap them.  Index -1 = outside the patch window (the patch's background colour), -2 = outside the source under the rotation (always 0).
// grid, plan and tables as aug_plan_kernel's.
template <class HW>
__global__ __launch_bounds__(128) void sat_plan_kernel(const int* __restrict__ geo, HW hw, int out_h, int out_w, int n_taps,
                                                       int* __restrict__ plan, int* __restrict__ ix, double* __restrict__ wx,
                                                       int* __restrict__ iy, double* __restrict__ wy, int* __restrict__ transposed) {
    const int b = (int)blockIdx.z, axis = (int)blockIdx.y;
    const int n_dst = axis == 0 ? out_w : out_h;
    const int i = (int)blockIdx.x * 128 + (int)threadIdx.x;
    const int* g = geo + (size_t)b * 12;
    const int Hs = hw.h(b), Ws = hw.w(b);                                        // the source image
    const int turns = g[7];
    const int Hr = (turns & 1) ? Ws : Hs, Wr = (turns & 1) ? Hs : Ws;            // the rotated image
    const int Hc = g[8], Wc = g[9];
    const AugPlan q = aug_plan_of(Hc, Wc, out_h, out_w, g[11], n_taps);
    if (axis == 0 && i == 0) {
        plan[b * 4] = q.kind; plan[b * 4 + 1] = q.area; plan[b * 4 + 2] = q.tx; plan[b * 4 + 3] = q.ty;
        transposed[b] = turns & 1;
    }
    if (i >= n_dst) return;
    const int n_src = axis == 0 ? Wc : Hc;
    int idx[64];
    double w[64];
    const int T = aug_axis_taps(q, axis, i, n_src, n_dst, idx, w);
    int* oi = (axis == 0 ? ix : iy) + ((size_t)b * n_dst + i) * n_taps;
    double* ow = (axis == 0 ? wx : wy) + ((size_t)b * n_dst + i) * n_taps;
    for (int t = 0; t < n_taps; ++t) {
        int j = idx[t < T ? t : T - 1];
        if (g[0]) {                                                               // the patch: the rotated image sits at (-top, -left)
            j += axis == 0 ? g[2] : g[1];
            if (j < 0 || j >= (axis == 0 ? Wr : Hr)) j = -1;
        }
        if (j >= 0) {
            bool column = axis == 0;                                              // does j address a source column?
            if (turns == 1) { column = axis == 1; if (axis == 1) j = Ws - j; }
            else if (turns == 2) j = (axis == 0 ? Ws : Hs) - j;
            else if (turns == 3) { column = axis == 1; if (axis == 0) j = Hs - j; }
            const int extent = column ? Ws : Hs;
            if (j >= extent) j = -2;                                              // the rotation's one border row / column
            else if (column ? g[5] : g[6]) j = extent - 1 - j;                    // the two flips
        }
        oi[t] = j;
        ow[t] = t < T ? w[t] : 0.0;
    }
}

}  // namespace ssdhip

using namespace ssdhip;

static int aug_params_from(const ssdhip_augment_params* q, AugParams& p);

// The whole batch on ONE generator stream, photometric decisions included (round 6; the reference's own generator semantics).
// mt_state / mt_state_out [625]; programs_ops [B][16] int32 + programs_args [B][16] float64: the per-image programs of
// ssdhip_image_program; the rest as ssdhip_ssd_augment_decide.  photo: probabilities and uniform ranges of RandomBrightness,
// RandomContrast, RandomSaturation, RandomHue (in that order); RandomChannelSwap must have probability 0 (SSDPhotometricDistortions).
extern "C" int ssdhip_ssd_augment_decide_stream(const ssdhip_augment_params* q, const ssdhip_augment_photo* photo, int B,
                                                const unsigned int* mt_state, const double* labels, const int* n_labels, int* programs_ops,
                                                double* programs_args, int* geometry, double* labels_out, int* n_labels_out,
                                                unsigned int* mt_state_out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!q || !photo || B <= 0 || !mt_state || !labels || !n_labels || !programs_ops || !programs_args || !geometry || !labels_out ||
        !n_labels_out || !mt_state_out)
        return SSDHIP_E_BADARG;
    if (photo->swap_prob != 0.0) return SSDHIP_E_BADARG;
    AugParams p;
    const int rc = aug_params_from(q, p);
    if (rc != SSDHIP_OK) return rc;
    AugPhoto ph;
    for (int i = 0; i < 4; ++i) {
        if (!(photo->prob[i] >= 0.0 && photo->prob[i] <= 1.0)) return SSDHIP_E_BADARG;
        ph.prob[i] = photo->prob[i]; ph.lo[i] = photo->lower[i]; ph.hi[i] = photo->upper[i];
    }
    ph.swap_prob = 0.0;
    hipLaunchKernelGGL(ssd_augment_stream_kernel<UniformHW>, dim3(1), dim3(64), 0, stream, p, ph, UniformHW{p.H, p.W}, B, mt_state, labels,
                       n_labels, programs_ops, programs_args, geometry, labels_out, n_labels_out, mt_state_out);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// The same walk over a ragged batch: image b's (H, W) from table_dev [B][4] int64 (byte offset, H, W, C) instead of params->img_height /
// img_width (which must still be positive: the largest H and W of the batch).  Same outputs.
extern "C" int ssdhip_ssd_augment_decide_stream_ragged(const ssdhip_augment_params* q, const ssdhip_augment_photo* photo, int B,
                                                       const long long* table_dev, const unsigned int* mt_state, const double* labels,
                                                       const int* n_labels, int* programs_ops, double* programs_args, int* geometry,
                                                       double* labels_out, int* n_labels_out, unsigned int* mt_state_out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!q || !photo || B <= 0 || !table_dev || !mt_state || !labels || !n_labels || !programs_ops || !programs_args || !geometry ||
        !labels_out || !n_labels_out || !mt_state_out)
        return SSDHIP_E_BADARG;
    if (photo->swap_prob != 0.0) return SSDHIP_E_BADARG;
    AugParams p;
    const int rc = aug_params_from(q, p);
    if (rc != SSDHIP_OK) return rc;
    AugPhoto ph;
    for (int i = 0; i < 4; ++i) {
        if (!(photo->prob[i] >= 0.0 && photo->prob[i] <= 1.0)) return SSDHIP_E_BADARG;
        ph.prob[i] = photo->prob[i]; ph.lo[i] = photo->lower[i]; ph.hi[i] = photo->upper[i];
    }
    ph.swap_prob = 0.0;
    hipLaunchKernelGGL(ssd_augment_stream_kernel<RaggedHW>, dim3(1), dim3(64), 0, stream, p, ph, RaggedHW{table_dev}, B, mt_state, labels,
                       n_labels, programs_ops, programs_args, geometry, labels_out, n_labels_out, mt_state_out);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_ssd_augment_decide(const ssdhip_augment_params* q, int B, const unsigned int* mt_state, const double* labels,
                                         const int* n_labels, int* geometry, double* labels_out, int* n_labels_out,
                                         unsigned int* mt_state_out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!q || B <= 0 || !mt_state || !labels || !n_labels || !geometry || !labels_out || !n_labels_out || !mt_state_out) return SSDHIP_E_BADARG;
    AugParams p;
    const int rc = aug_params_from(q, p);
    if (rc != SSDHIP_OK) return rc;
    hipLaunchKernelGGL(ssd_augment_decide_kernel, dim3((unsigned)B), dim3(64), 0, stream, p, mt_state, labels, n_labels, geometry,
                       labels_out, n_labels_out, mt_state_out);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

static int aug_params_from(const ssdhip_augment_params* q, AugParams& p) {
    if (q->img_height <= 0 || q->img_width <= 0 || q->out_height <= 0 || q->out_width <= 0) return SSDHIP_E_BADARG;
    if (q->n_bounds < 1 || q->n_bounds > 8 || q->n_modes < 1 || q->n_modes > 8 || q->n_trials < 1) return SSDHIP_E_BADARG;
    if (!(q->expand_min_scale >= 1.0) || !(q->expand_max_scale > q->expand_min_scale)) return SSDHIP_E_BADARG;       // a canvas, never a crop
    if (!(q->crop_min_scale > 0.0) || !(q->crop_max_scale <= 1.0) || !(q->crop_max_scale > q->crop_min_scale)) return SSDHIP_E_BADARG;
    p.H = q->img_height; p.W = q->img_width;
    p.exp_prob = q->expand_prob; p.exp_min = q->expand_min_scale; p.exp_max = q->expand_max_scale;
    p.crop_prob = q->crop_prob; p.crop_min = q->crop_min_scale; p.crop_max = q->crop_max_scale;
    p.ar_min = q->crop_min_aspect_ratio; p.ar_max = q->crop_max_aspect_ratio;
    p.n_trials = q->n_trials; p.n_bounds = q->n_bounds;
    for (int i = 0; i < 8; ++i) { p.cdf[i] = q->bound_cdf[i]; p.lower[i] = q->bound_lower[i]; p.upper[i] = q->bound_upper[i]; p.modes[i] = q->interpolation_modes[i]; }
    p.flip_prob = q->flip_prob; p.n_modes = q->n_modes; p.out_h = q->out_height; p.out_w = q->out_width;
    p.max_rounds = q->max_rounds > 0 ? q->max_rounds : 100000;
    return SSDHIP_OK;
}

extern "C" int ssdhip_augment_plans(const int* geometry_dev, int B, int H, int W, int out_h, int out_w, int n_taps, int* plan_dev,
                                    int* ix_dev, double* wx_dev, int* iy_dev, double* wy_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!geometry_dev || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || B <= 0 || B > 65535 || H <= 0 || W <= 0 || out_h <= 0 ||
        out_w <= 0)
        return SSDHIP_E_BADARG;
    if (n_taps < 8 || n_taps > 64) return SSDHIP_E_BADARG;                       // Lanczos-4 needs eight
    const int n = out_h > out_w ? out_h : out_w;
    hipLaunchKernelGGL(aug_plan_kernel<UniformHW>, dim3((unsigned)((n + 127) / 128), 2, (unsigned)B), dim3(128), 0, stream, geometry_dev,
                       UniformHW{H, W}, out_h, out_w, n_taps, plan_dev, ix_dev, wx_dev, iy_dev, wy_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// ssdhip_augment_plans for a ragged batch: image b's canvas bounds from table_dev [B][4] int64 (byte offset, H, W, C); the plans index
// each image's own rows / columns (ssdhip_image_resize_gather_ragged_u8).
extern "C" int ssdhip_augment_plans_ragged(const int* geometry_dev, const long long* table_dev, int B, int out_h, int out_w, int n_taps,
                                           int* plan_dev, int* ix_dev, double* wx_dev, int* iy_dev, double* wy_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!geometry_dev || !table_dev || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || B <= 0 || B > 65535 || out_h <= 0 ||
        out_w <= 0)
        return SSDHIP_E_BADARG;
    if (n_taps < 8 || n_taps > 64) return SSDHIP_E_BADARG;
    const int n = out_h > out_w ? out_h : out_w;
    hipLaunchKernelGGL(aug_plan_kernel<RaggedHW>, dim3((unsigned)((n + 127) / 128), 2, (unsigned)B), dim3(128), 0, stream, geometry_dev,
                       RaggedHW{table_dev}, out_h, out_w, n_taps, plan_dev, ix_dev, wx_dev, iy_dev, wy_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// ---- DataAugmentationConstantInputSize: the decisions of a batch (seeded: B states; stream: one) and the warp launch's tables -----------
static int const_params_from(const ssdhip_const_augment_params* q, ConstAugParams& p) {
    const auto prob = [](double v) { return v >= 0.0 && v <= 1.0; };
    if (q->img_height <= 0 || q->img_width <= 0 || q->img_height > 32767 || q->img_width > 32767) return SSDHIP_E_BADARG;
    for (int i = 0; i < 4; ++i)
        if (!prob(q->photo_prob[i]) || !(q->photo_upper[i] >= q->photo_lower[i])) return SSDHIP_E_BADARG;
    if (!prob(q->translate_prob) || !prob(q->zoom_in_prob) || !prob(q->zoom_out_prob) || !prob(q->flip_prob)) return SSDHIP_E_BADARG;
    if (!(q->dy_min >= 0.0) || !(q->dy_max >= q->dy_min) || !(q->dx_min >= 0.0) || !(q->dx_max >= q->dx_min)) return SSDHIP_E_BADARG;
    if (!(q->zoom_in_min > 0.0) || !(q->zoom_in_max >= q->zoom_in_min) || !(q->zoom_out_min > 0.0) || !(q->zoom_out_max >= q->zoom_out_min))
        return SSDHIP_E_BADARG;
    if (q->n_trials < 1 || q->n_trials > 64 || q->n_boxes_min < 1) return SSDHIP_E_BADARG;
    if (!(q->validator_upper >= q->validator_lower) || !(q->filter_upper >= q->filter_lower) || !(q->filter_min_area == q->filter_min_area))
        return SSDHIP_E_BADARG;
    p.H = q->img_height; p.W = q->img_width;
    for (int i = 0; i < 4; ++i) { p.ph_prob[i] = q->photo_prob[i]; p.ph_lo[i] = q->photo_lower[i]; p.ph_hi[i] = q->photo_upper[i]; }
    p.tr_prob = q->translate_prob; p.dy_lo = q->dy_min; p.dy_hi = q->dy_max; p.dx_lo = q->dx_min; p.dx_hi = q->dx_max;
    p.zin_prob = q->zoom_in_prob; p.zin_lo = q->zoom_in_min; p.zin_hi = q->zoom_in_max;
    p.zout_prob = q->zoom_out_prob; p.zout_lo = q->zoom_out_min; p.zout_hi = q->zoom_out_max;
    p.flip_prob = q->flip_prob;
    p.n_trials = q->n_trials; p.clip = q->clip_boxes != 0; p.n_min = q->n_boxes_min;
    p.val_lo = q->validator_lower; p.val_hi = q->validator_upper;
    p.flt_lo = q->filter_lower; p.flt_hi = q->filter_upper; p.min_area = q->filter_min_area;
    return SSDHIP_OK;
}

template <bool STREAM>
static int const_decide(const ssdhip_const_augment_params* q, int B, const unsigned int* mt_state, const double* labels, const int* n_labels,
                        int* programs_ops, double* programs_args, double* geometry, double* labels_out, int* n_labels_out,
                        unsigned int* mt_state_out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!q || B <= 0 || !mt_state || !labels || !n_labels || !programs_ops || !programs_args || !geometry || !labels_out || !n_labels_out ||
        !mt_state_out)
        return SSDHIP_E_BADARG;
    ConstAugParams p;
    const int rc = const_params_from(q, p);
    if (rc != SSDHIP_OK) return rc;
    hipLaunchKernelGGL(const_augment_decide_kernel<STREAM>, dim3(STREAM ? 1u : (unsigned)B), dim3(64), 0, stream, p, B, mt_state, labels,
                       n_labels, programs_ops, programs_args, geometry, labels_out, n_labels_out, mt_state_out);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_const_augment_decide(const ssdhip_const_augment_params* params, int B, const unsigned int* mt_state,
                                           const double* labels, const int* n_labels, int* programs_ops, double* programs_args,
                                           double* geometry, double* labels_out, int* n_labels_out, unsigned int* mt_state_out,
                                           void* stream) {
    return const_decide<false>(params, B, mt_state, labels, n_labels, programs_ops, programs_args, geometry, labels_out, n_labels_out,
                               mt_state_out, stream);
}

extern "C" int ssdhip_const_augment_decide_stream(const ssdhip_const_augment_params* params, int B, const unsigned int* mt_state,
                                                  const double* labels, const int* n_labels, int* programs_ops, double* programs_args,
                                                  double* geometry, double* labels_out, int* n_labels_out, unsigned int* mt_state_out,
                                                  void* stream) {
    return const_decide<true>(params, B, mt_state, labels, n_labels, programs_ops, programs_args, geometry, labels_out, n_labels_out,
                              mt_state_out, stream);
}

extern "C" int ssdhip_const_augment_plans(const double* geometry_dev, int B, int H, int W, int* geo_dev, int* xtab_dev, int* ytab_dev,
                                          void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!geometry_dev || !geo_dev || !xtab_dev || !ytab_dev || B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > 32767 || W > 32767)
        return SSDHIP_E_BADARG;
    const int n = H > W ? H : W;
    hipLaunchKernelGGL(const_plan_kernel, dim3((unsigned)((n + 127) / 128), 2, (unsigned)B), dim3(128), 0, stream, geometry_dev, H, W,
                       geo_dev, xtab_dev, ytab_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

// ---- DataAugmentationVariableInputSize: the decisions of a batch (seeded: B states; stream: one), uniform or ragged sizes ----------------
static int var_params_from(const ssdhip_var_augment_params* q, bool ragged, int n_boxes_max, VarAugParams& p) {
    const auto prob = [](double v) { return v >= 0.0 && v <= 1.0; };
    if (!ragged && (q->img_height <= 0 || q->img_width <= 0)) return SSDHIP_E_BADARG;
    if (n_boxes_max < 0 || n_boxes_max > AUG_MAXG) return SSDHIP_E_BADARG;
    for (int i = 0; i < 4; ++i)
        if (!prob(q->photo_prob[i]) || !(q->photo_upper[i] >= q->photo_lower[i])) return SSDHIP_E_BADARG;
    if (!prob(q->patch_prob) || !prob(q->flip_prob)) return SSDHIP_E_BADARG;
    if (!(q->min_scale > 0.0) || !(q->max_scale >= q->min_scale) || !(q->min_aspect_ratio > 0.0) ||
        !(q->max_aspect_ratio >= q->min_aspect_ratio))
        return SSDHIP_E_BADARG;
    if (q->n_trials < 0 || q->n_boxes_min < 0) return SSDHIP_E_BADARG;
    if (q->criterion != SSDHIP_VAR_AUG_CENTER_POINT && q->criterion != SSDHIP_VAR_AUG_IOU && q->criterion != SSDHIP_VAR_AUG_AREA)
        return SSDHIP_E_BADARG;
    if (!(q->validator_upper >= q->validator_lower) || !(q->filter_upper >= q->filter_lower) || !(q->resize_min_area == q->resize_min_area))
        return SSDHIP_E_BADARG;
    if (q->out_height <= 0 || q->out_width <= 0 || q->interpolation < 0 || q->interpolation > 4) return SSDHIP_E_BADARG;
    for (int i = 0; i < 4; ++i) { p.ph_prob[i] = q->photo_prob[i]; p.ph_lo[i] = q->photo_lower[i]; p.ph_hi[i] = q->photo_upper[i]; }
    p.patch_prob = q->patch_prob; p.scale_lo = q->min_scale; p.scale_hi = q->max_scale;
    p.ar_lo = q->min_aspect_ratio; p.ar_hi = q->max_aspect_ratio;
    p.n_trials = q->n_trials > 1 ? q->n_trials : 1;                          // max(1, n_trials_max)
    p.clip = q->clip_boxes != 0; p.criterion = q->criterion; p.n_min = q->n_boxes_min;
    p.val_lo = q->validator_lower; p.val_hi = q->validator_upper; p.flt_lo = q->filter_lower; p.flt_hi = q->filter_upper;
    p.flip_prob = q->flip_prob;
    p.out_h = q->out_height; p.out_w = q->out_width; p.interp = q->interpolation; p.min_area = q->resize_min_area;
    return SSDHIP_OK;
}

template <bool STREAM>
static int var_decide(const ssdhip_var_augment_params* q, int B, int n_boxes_max, const long long* table_dev, const unsigned int* mt_state,
                      const double* labels, const int* n_labels, int* programs_ops, double* programs_args, int* geometry,
                      double* labels_out, int* n_labels_out, unsigned int* mt_state_out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!q || B <= 0 || !mt_state || !labels || !n_labels || !programs_ops || !programs_args || !geometry || !labels_out || !n_labels_out ||
        !mt_state_out)
        return SSDHIP_E_BADARG;
    VarAugParams p;
    const int rc = var_params_from(q, table_dev != nullptr, n_boxes_max, p);
    if (rc != SSDHIP_OK) return rc;
    const dim3 grid(STREAM ? 1u : (unsigned)B);
    if (table_dev)
        hipLaunchKernelGGL((var_augment_decide_kernel<STREAM, RaggedHW>), grid, dim3(64), 0, stream, p, RaggedHW{table_dev}, B, mt_state,
                           labels, n_labels, programs_ops, programs_args, geometry, labels_out, n_labels_out, mt_state_out);
    else
        hipLaunchKernelGGL((var_augment_decide_kernel<STREAM, UniformHW>), grid, dim3(64), 0, stream, p,
                           UniformHW{q->img_height, q->img_width}, B, mt_state, labels, n_labels, programs_ops, programs_args, geometry,
                           labels_out, n_labels_out, mt_state_out);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_var_augment_decide(const ssdhip_var_augment_params* params, int B, int n_boxes_max, const long long* table_dev,
                                         const unsigned int* mt_state, const double* labels, const int* n_labels, int* programs_ops,
                                         double* programs_args, int* geometry, double* labels_out, int* n_labels_out,
                                         unsigned int* mt_state_out, void* stream) {
    return var_decide<false>(params, B, n_boxes_max, table_dev, mt_state, labels, n_labels, programs_ops, programs_args, geometry,
                             labels_out, n_labels_out, mt_state_out, stream);
}

extern "C" int ssdhip_var_augment_decide_stream(const ssdhip_var_augment_params* params, int B, int n_boxes_max,
                                                const unsigned int* mt_state, const double* labels, const int* n_labels, int* programs_ops,
                                                double* programs_args, int* geometry, double* labels_out, int* n_labels_out,
                                                unsigned int* mt_state_out, void* stream) {
    return var_decide<true>(params, B, n_boxes_max, nullptr, mt_state, labels, n_labels, programs_ops, programs_args, geometry, labels_out,
                            n_labels_out, mt_state_out, stream);
}

extern "C" int ssdhip_var_augment_decide_stream_ragged(const ssdhip_var_augment_params* params, int B, int n_boxes_max,
                                                       const long long* table_dev, const unsigned int* mt_state, const double* labels,
                                                       const int* n_labels, int* programs_ops, double* programs_args, int* geometry,
                                                       double* labels_out, int* n_labels_out, unsigned int* mt_state_out, void* stream) {
    if (!table_dev) return SSDHIP_E_BADARG;
    return var_decide<true>(params, B, n_boxes_max, table_dev, mt_state, labels, n_labels, programs_ops, programs_args, geometry, labels_out,
                            n_labels_out, mt_state_out, stream);
}

// ---- DataAugmentationSatellite: the decisions of a batch (seeded: B states; stream: one), uniform or ragged sizes, and its plans ----------
template <bool STREAM>
static int sat_decide(const ssdhip_sat_augment_params* q, int B, int n_boxes_max, const long long* table_dev, const int* turns_dev,
                      const unsigned int* mt_state, const double* labels, const int* n_labels, int* programs_ops, double* programs_args,
                      int* geometry, double* labels_out, int* n_labels_out, unsigned int* mt_state_out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!q || B <= 0 || !turns_dev || !mt_state || !labels || !n_labels || !programs_ops || !programs_args || !geometry || !labels_out ||
        !n_labels_out || !mt_state_out)
        return SSDHIP_E_BADARG;
    if (!(q->vflip_prob >= 0.0 && q->vflip_prob <= 1.0) || !(q->rotate_prob >= 0.0 && q->rotate_prob <= 1.0)) return SSDHIP_E_BADARG;
    SatAugParams p;
    const int rc = var_params_from(&q->var, table_dev != nullptr, n_boxes_max, p.v);
    if (rc != SSDHIP_OK) return rc;
    p.vflip_prob = q->vflip_prob; p.rot_prob = q->rotate_prob;
    const dim3 grid(STREAM ? 1u : (unsigned)B);
    if (table_dev)
        hipLaunchKernelGGL((sat_augment_decide_kernel<STREAM, RaggedHW>), grid, dim3(64), 0, stream, p, RaggedHW{table_dev}, B, turns_dev,
                           mt_state, labels, n_labels, programs_ops, programs_args, geometry, labels_out, n_labels_out, mt_state_out);
    else
        hipLaunchKernelGGL((sat_augment_decide_kernel<STREAM, UniformHW>), grid, dim3(64), 0, stream, p,
                           UniformHW{q->var.img_height, q->var.img_width}, B, turns_dev, mt_state, labels, n_labels, programs_ops,
                           programs_args, geometry, labels_out, n_labels_out, mt_state_out);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_sat_augment_decide(const ssdhip_sat_augment_params* params, int B, int n_boxes_max, const long long* table_dev,
                                         const int* turns_dev, const unsigned int* mt_state, const double* labels, const int* n_labels,
                                         int* programs_ops, double* programs_args, int* geometry, double* labels_out, int* n_labels_out,
                                         unsigned int* mt_state_out, void* stream) {
    return sat_decide<false>(params, B, n_boxes_max, table_dev, turns_dev, mt_state, labels, n_labels, programs_ops, programs_args, geometry,
                             labels_out, n_labels_out, mt_state_out, stream);
}

extern "C" int ssdhip_sat_augment_decide_stream(const ssdhip_sat_augment_params* params, int B, int n_boxes_max, const int* turns_dev,
                                                const unsigned int* mt_state, const double* labels, const int* n_labels, int* programs_ops,
                                                double* programs_args, int* geometry, double* labels_out, int* n_labels_out,
                                                unsigned int* mt_state_out, void* stream) {
    return sat_decide<true>(params, B, n_boxes_max, nullptr, turns_dev, mt_state, labels, n_labels, programs_ops, programs_args, geometry,
                            labels_out, n_labels_out, mt_state_out, stream);
}

extern "C" int ssdhip_sat_augment_decide_stream_ragged(const ssdhip_sat_augment_params* params, int B, int n_boxes_max,
                                                       const long long* table_dev, const int* turns_dev, const unsigned int* mt_state,
                                                       const double* labels, const int* n_labels, int* programs_ops, double* programs_args,
                                                       int* geometry, double* labels_out, int* n_labels_out, unsigned int* mt_state_out,
                                                       void* stream) {
    if (!table_dev) return SSDHIP_E_BADARG;
    return sat_decide<true>(params, B, n_boxes_max, table_dev, turns_dev, mt_state, labels, n_labels, programs_ops, programs_args, geometry,
                            labels_out, n_labels_out, mt_state_out, stream);
}

extern "C" int ssdhip_sat_augment_plans(const int* geometry_dev, int B, int H, int W, int out_h, int out_w, int n_taps, int* plan_dev,
                                        int* ix_dev, double* wx_dev, int* iy_dev, double* wy_dev, int* transposed_dev, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!geometry_dev || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || !transposed_dev || B <= 0 || B > 65535 || H <= 0 ||
        W <= 0 || out_h <= 0 || out_w <= 0)
        return SSDHIP_E_BADARG;
    if (n_taps < 8 || n_taps > 64) return SSDHIP_E_BADARG;
    const int n = out_h > out_w ? out_h : out_w;
    hipLaunchKernelGGL(sat_plan_kernel<UniformHW>, dim3((unsigned)((n + 127) / 128), 2, (unsigned)B), dim3(128), 0, stream, geometry_dev,
                       UniformHW{H, W}, out_h, out_w, n_taps, plan_dev, ix_dev, wx_dev, iy_dev, wy_dev, transposed_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}

extern "C" int ssdhip_sat_augment_plans_ragged(const int* geometry_dev, const long long* table_dev, int B, int out_h, int out_w, int n_taps,
                                               int* plan_dev, int* ix_dev, double* wx_dev, int* iy_dev, double* wy_dev, int* transposed_dev,
                                               void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!geometry_dev || !table_dev || !plan_dev || !ix_dev || !wx_dev || !iy_dev || !wy_dev || !transposed_dev || B <= 0 || B > 65535 ||
        out_h <= 0 || out_w <= 0)
        return SSDHIP_E_BADARG;
    if (n_taps < 8 || n_taps > 64) return SSDHIP_E_BADARG;
    const int n = out_h > out_w ? out_h : out_w;
    hipLaunchKernelGGL(sat_plan_kernel<RaggedHW>, dim3((unsigned)((n + 127) / 128), 2, (unsigned)B), dim3(128), 0, stream, geometry_dev,
                       RaggedHW{table_dev}, out_h, out_w, n_taps, plan_dev, ix_dev, wx_dev, iy_dev, wy_dev, transposed_dev);
    return hipGetLastError() == hipSuccess ? SSDHIP_OK : SSDHIP_E_LAUNCH;
}
