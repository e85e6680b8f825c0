// libctdet: the augmentation DECISIONS and the box targets of data/data_augment.py `preproc.decide` on the device.
// ct_preproc.hip produces the pixels from a ct_aug_plan_record per image; until here the plan came from the host's scalar
// rejection sampler.  ct_aug_plan draws the same decisions from a counter-based generator (Philox4x32-10, the draw
// table of include/ctdet.h), transforms the boxes and packs them as ct_match_batched reads them.
//   launch 1  aug_plan_kernel: one wave per sample, lanes = trials of a crop / expand round; the lowest passing lane
//             (ballot) wins and its draw is broadcast; the kept rows are compacted by ballot prefix counts into the
//             sample's workspace slot.
//   launch 2  aug_pack_kernel: one workgroup scans the per-sample counts into gt_off_out, refuses samples whose image
//             index decreases, copies the rows and writes the status words.
// ct_aug_plan_mosaic runs the same two launches over 4 samples per image with aug_mosaic_kernel between them: the four
// samples' rows are mapped into the tiles of one composed image (include/ctdet.h MOSAIC).
// All decision arithmetic is fp64 with +, -, *, /, sqrt, comparisons and truncation only (compiled with contraction
// off), the sequence ctdet/aug_plan_ref.py evaluates in numpy: both give the same bytes.
#include "ct_common.h"
#include "ct_aug_draw.h"
#include <algorithm>

namespace {

using namespace ctdet::aug;                 // philox, the draw rules, block_scan

using AugPlan = ct_aug_plan_record;         // one image's decisions (include/ctdet.h)

struct Interp5 { int v[5]; };
struct Fill3 { float v[3]; };

constexpr int SLOT_MISC = 0, SLOT_CROP = 0x100, SLOT_EXPAND = 0x200;
constexpr int LANE_COINS = 0, LANE_PARAMS = 1, LANE_MISC = 2, LANE_MODE = 63;
constexpr int CROP_TRIALS = 50, CROP_ROUNDS = 256, EXPAND_ROUNDS = 64;

__device__ __forceinline__ void identity_plan(AugPlan& p, int H, int W)
{
    p.H = H; p.W = W;
    p.crop_l = 0; p.crop_t = 0; p.crop_w = W; p.crop_h = H;
    p.exp_w = W; p.exp_h = H; p.exp_left = 0; p.exp_top = 0;
    p.mirror = 0; p.interp = 0; p.flags = 0; p.hue_delta = 0;
    p.beta = 0.f; p.alpha = 1.f; p.sat_alpha = 1.f;
}

struct Geometry {           // what the boxes go through after the draws
    int cropped, l, t, w, h;
    int expanded, ew, eh, left, top;
    int mirror;
};

// box j through crop -> canvas -> mirror -> normalisation (preproc.decide); false when the row is not kept
__device__ inline bool transform_row(const float* __restrict__ bx, const Geometry& g, double (&o)[5])
{
    double x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
    o[4] = bx[4];
    bool keep = true;
    if (g.cropped) {
        const double cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;
        const double rl = g.l, rt = g.t, rr = g.l + g.w, rb = g.t + g.h;
        keep = rl < cx && cx < rr && rt < cy && cy < rb;
        x1 = fmax(x1, rl) - rl; y1 = fmax(y1, rt) - rt;
        x2 = fmin(x2, rr) - rl; y2 = fmin(y2, rb) - rt;
    }
    if (g.expanded) { x1 += g.left; y1 += g.top; x2 += g.left; y2 += g.top; }
    if (g.mirror) { const double a = g.ew - x2, b = g.ew - x1; x1 = a; x2 = b; }
    x1 = x1 / g.ew; y1 = y1 / g.eh; x2 = x2 / g.ew; y2 = y2 / g.eh;
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
    return keep && fmin(x2 - x1, y2 - y1) > 0.01;
}

// One wave per sample.  Everything but the per-lane trial is wave-uniform.
__global__ __launch_bounds__(64) void aug_plan_kernel(const ct_aug_sample* __restrict__ samples, int num_samples,
                                                      const float* __restrict__ boxes, int total_boxes, int num_images,
                                                      int max_gt, unsigned long long seed, double p_expand, Interp5 interp,
                                                      Fill3 fill, AugPlan* __restrict__ plans, int* __restrict__ counts,
                                                      float* __restrict__ rows)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= num_samples) return;
    const ct_aug_sample sm = samples[s];
    AugPlan plan;
    plan.src_off = sm.src_off;
    plan.fill[0] = fill.v[0]; plan.fill[1] = fill.v[1]; plan.fill[2] = fill.v[2];
    plan.pad0 = 0.f; plan.pad1 = 0.f;
    if (sm.image < 0 || sm.image >= num_images || sm.H < 1 || sm.W < 1) {       // refused: identity plan, no rows
        identity_plan(plan, max(sm.H, 1), max(sm.W, 1));
        if (lane == 0) { plans[s] = plan; counts[s] = -1; }
        return;
    }
    const int H = sm.H, W = sm.W, cls = sm.cls;
    const int b0 = min(max(sm.box_begin, 0), total_boxes), b1 = min(max(sm.box_end, 0), total_boxes);
    const int n = min(max(b1 - b0, 0), max_gt);
    const float* __restrict__ bx = boxes + (size_t)b0 * 5;
    const unsigned long long sid = sm.sample_id;

    Geometry g;
    g.cropped = 0; g.l = 0; g.t = 0; g.w = W; g.h = H;
    // ---- crop (data_augment.py _crop)
    if (n > 0) {
        for (int r = 0; r < CROP_ROUNDS; ++r) {
            const int mode = randrange(7, philox(seed, sid, SLOT_CROP + r, LANE_MODE).w[0]);
            if (mode == 0) break;
            // CROP_MODES: (min_iou, None) for modes 1..5, (None, None) for mode 6; no mode has an upper bound
            const double min_iou = mode == 1 ? 0.1 : mode == 2 ? 0.3 : mode == 3 ? 0.5 : mode == 4 ? 0.7 :
                                   mode == 5 ? 0.9 : -__builtin_inf();
            const Words d = philox(seed, sid, SLOT_CROP + r, lane);
            const double scale = uniform(0.3, 1.0, d.w[0]);
            const double lo = fmax(0.5, scale * scale), hi = fmin(2.0, 1.0 / scale / scale);
            const double ratio = sqrt(lo + (hi - lo) * unit(d.w[1]));
            const int w = (int)(scale * ratio * W), h = (int)(scale / ratio * H);
            bool ok = lane < CROP_TRIALS && w >= 1 && h >= 1 && w < W && h < H;
            const int l = randrange(ok ? W - w : 1, d.w[2]), t = randrange(ok ? H - h : 1, d.w[3]);
            if (ok) {
                const double rl = l, rt = t, rr = l + w, rb = t + h;
                const double area_b = (rr - rl) * (rb - rt);
                double mn = __builtin_inf(), mx = -__builtin_inf();
                bool any_in = false, any_cls = false;
                for (int j = 0; j < n; ++j) {
                    const double x1 = bx[j * 5], y1 = bx[j * 5 + 1], x2 = bx[j * 5 + 2], y2 = bx[j * 5 + 3];
                    const double ltx = fmax(x1, rl), lty = fmax(y1, rt), rbx = fmin(x2, rr), rby = fmin(y2, rb);
                    const double area_i = (rbx - ltx) * (rby - lty) * ((ltx < rbx && lty < rby) ? 1.0 : 0.0);
                    const double area_a = (x2 - x1) * (y2 - y1);
                    const double iou = area_i / (area_a + area_b - area_i);
                    if (iou < mn) mn = iou;
                    if (iou > mx) mx = iou;
                    const double cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;
                    const bool in = rl < cx && cx < rr && rt < cy && cy < rb;
                    any_in |= in;
                    any_cls |= in && (double)bx[j * 5 + 4] == (double)(cls + 1);
                }
                ok = min_iou <= mn && mx <= __builtin_inf() && any_in && (cls < 0 || any_cls);
            }
            const unsigned long long mask = __ballot(ok);
            if (mask) {
                const int win = __ffsll((long long)mask) - 1;
                g.cropped = 1;
                g.l = __shfl(l, win); g.t = __shfl(t, win); g.w = __shfl(w, win); g.h = __shfl(h, win);
                break;
            }
        }
    }
    // ---- distort (_distort): four coins, four parameters
    const Words coin = philox(seed, sid, SLOT_MISC, LANE_COINS), prm = philox(seed, sid, SLOT_MISC, LANE_PARAMS);
    const Words misc = philox(seed, sid, SLOT_MISC, LANE_MISC);
    int flags = 0, hue = 0;
    double beta = 0.0, alpha = 1.0, sat = 1.0;
    if (coin.w[0] >> 31) { flags |= 1; beta = uniform(-32.0, 32.0, prm.w[0]); }
    if (coin.w[1] >> 31) { flags |= 2; alpha = uniform(0.5, 1.5, prm.w[1]); }
    if (coin.w[2] >> 31) { flags |= 4; hue = -18 + randrange(37, prm.w[2]); }
    if (coin.w[3] >> 31) { flags |= 8; sat = uniform(0.5, 1.5, prm.w[3]); }
    // ---- expand (_expand) on the crop
    g.expanded = 0; g.ew = g.w; g.eh = g.h; g.left = 0; g.top = 0;
    if (!(unit(misc.w[0]) > p_expand)) {
        for (int r = 0; r < EXPAND_ROUNDS; ++r) {
            const Words d = philox(seed, sid, SLOT_EXPAND + r, lane);
            const double scale = uniform(1.0, 4.0, d.w[0]);
            const double lo = fmax(0.5, 1.0 / scale / scale), hi = fmin(2.0, scale * scale);
            const double ratio = sqrt(lo + (hi - lo) * unit(d.w[1]));
            const double ws = scale * ratio, hs = scale / ratio;
            const bool ok = !(ws < 1 || hs < 1);
            const int w = (int)(ws * g.w), h = (int)(hs * g.h);
            const int left = randrange(ok ? w - g.w + 1 : 1, d.w[2]), top = randrange(ok ? h - g.h + 1 : 1, d.w[3]);
            const unsigned long long mask = __ballot(ok);
            if (mask) {
                const int win = __ffsll((long long)mask) - 1;
                g.expanded = 1;
                g.ew = __shfl(w, win); g.eh = __shfl(h, win); g.left = __shfl(left, win); g.top = __shfl(top, win);
                break;
            }
        }
    }
    g.mirror = (int)(misc.w[1] >> 31);
    // ---- targets, pass 1: how many rows are kept, and is the constrained class among them
    int kept = 0;
    bool cls_kept = false;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        double o[5];
        const bool keep = j < n && transform_row(bx + (size_t)j * 5, g, o);
        kept += __popcll(__ballot(keep));
        cls_kept |= __ballot(keep && o[4] == (double)(cls + 1)) != 0;
    }
    const bool fallback = kept == 0 || (cls >= 0 && !cls_kept);
    // ---- pass 2: the rows, compacted in input order into the sample's slot
    float* __restrict__ out = rows + (size_t)s * max_gt * 6;
    int at = 0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        double o[5];
        bool keep = false;
        if (j < n) {
            if (fallback) {
                const float* q = bx + (size_t)j * 5;
                o[0] = (double)q[0] / W; o[1] = (double)q[1] / H; o[2] = (double)q[2] / W; o[3] = (double)q[3] / H;
                o[4] = q[4];
                keep = true;
            } else {
                keep = transform_row(bx + (size_t)j * 5, g, o);
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int k = at + __popcll(mask & ((1ull << lane) - 1ull));
            double label = o[4];
            if ((sm.flags & 2) && k >= 1) label = -1.0;
            float weight = sm.weight;
            if ((sm.flags & 1) && label == -1.0) weight = 0.f;
            float* q = out + (size_t)k * 6;
            q[0] = (float)o[0]; q[1] = (float)o[1]; q[2] = (float)o[2]; q[3] = (float)o[3];
            q[4] = (float)label; q[5] = weight;
        }
        at += __popcll(mask);
    }
    if (lane == 0) {
        if (fallback) {
            identity_plan(plan, H, W);
            plan.interp = interp.v[randrange(5, misc.w[3])];
        } else {
            plan.H = H; plan.W = W;
            plan.crop_l = g.l; plan.crop_t = g.t; plan.crop_w = g.w; plan.crop_h = g.h;
            plan.exp_w = g.ew; plan.exp_h = g.eh; plan.exp_left = g.left; plan.exp_top = g.top;
            plan.mirror = g.mirror; plan.interp = interp.v[randrange(5, misc.w[2])];
            plan.flags = flags; plan.hue_delta = hue;
            plan.beta = (float)beta; plan.alpha = (float)alpha; plan.sat_alpha = (float)sat;
        }
        plans[s] = plan;
        counts[s] = at;
    }
}

// One workgroup: a thread owns one sample of the current chunk of PACK_THREADS.  Rows of refused samples are
// dropped, rows past truths_cap are dropped; gt_off[b] = rows (capped) of the images before b.
__global__ __launch_bounds__(PACK_THREADS) void aug_pack_kernel(const ct_aug_sample* __restrict__ samples, int num_samples,
                                                                int num_images, int max_gt, AugPlan* __restrict__ plans,
                                                                const int* __restrict__ counts,
                                                                const float* __restrict__ rows, float* __restrict__ truths,
                                                                int truths_cap, int* __restrict__ gt_off,
                                                                int* __restrict__ status)
{
    __shared__ int sh[PACK_THREADS];
    __shared__ int carry_max, carry_sum, n_bad, n_dropped;
    const int tid = threadIdx.x;
    if (tid == 0) { carry_max = -1; carry_sum = 0; n_bad = 0; n_dropped = 0; }
    __syncthreads();
    for (int base = 0; base < num_samples; base += PACK_THREADS) {
        const int i = base + tid;
        const bool live = i < num_samples;
        int img = -1, cnt = 0;
        bool bad = false;
        if (live) {
            const int im = samples[i].image, c = counts[i];
            if (im >= 0 && im < num_images) img = im;
            bad = c < 0;
            cnt = min(max(c, 0), max_gt);
        }
        const int cmax = carry_max, csum = carry_sum;
        const int incl_max = block_scan<true>(img, sh);
        const int prev = max(cmax, tid > 0 ? sh[tid - 1] : -1);        // largest image index before this sample
        __syncthreads();
        if (live && img >= 0 && img < prev) {                          // decreasing: refused here
            bad = true;
            cnt = 0;
            AugPlan p = plans[i];
            identity_plan(p, p.H, p.W);
            plans[i] = p;
        }
        if (bad) { cnt = 0; atomicAdd(&n_bad, 1); }
        const int incl_sum = block_scan<false>(cnt, sh);
        const int off = csum + incl_sum - cnt;
        if (live && img > prev)
            for (int b = prev + 1; b <= img; ++b) gt_off[b] = min(off, truths_cap);
        const float* __restrict__ src = rows + (size_t)i * max_gt * 6;
        int dropped = 0;
        for (int j = 0; j < cnt; ++j) {
            const int dst = off + j;
            if (dst < truths_cap) {
                for (int c = 0; c < 6; ++c) truths[(size_t)dst * 6 + c] = src[j * 6 + c];
            } else {
                ++dropped;
            }
        }
        if (dropped) atomicAdd(&n_dropped, dropped);
        __syncthreads();
        if (tid == PACK_THREADS - 1) { carry_max = max(cmax, incl_max); carry_sum = csum + incl_sum; }
        __syncthreads();
    }
    const int total = carry_sum, last = carry_max;
    for (int b = last + 1 + tid; b <= num_images; b += PACK_THREADS) gt_off[b] = min(total, truths_cap);
    __syncthreads();
    if (tid == 0) {
        status[0] = (n_bad ? 1 : 0) | (n_dropped ? 2 : 0);
        status[1] = n_bad;
        status[2] = n_dropped;
        status[3] = total;
    }
}

// Mosaic, between the two launches above: one wave per image composes its four samples (include/ctdet.h MOSAIC).
// It draws the meeting point, writes the four tiles, refuses a sample whose image field is not its group, maps each
// sample's rows from its own canvas into its tile (fp64, operation by operation), filters them in units of the output
// image and compacts them in place in the sample's workspace slot, and rewrites the per-sample counts.  `fixed` gets
// the sample table with image = s / 4, which is what aug_pack_kernel then scans: a foreign image field cannot make
// it refuse a neighbour.
constexpr int SLOT_MOSAIC = 0x300;

__device__ __forceinline__ bool mosaic_row(const float* q, const ct_mosaic_tile& t, int S, double (&o)[4])
{
    o[0] = (t.x0 + (double)q[0] * t.w) / S; o[1] = (t.y0 + (double)q[1] * t.h) / S;
    o[2] = (t.x0 + (double)q[2] * t.w) / S; o[3] = (t.y0 + (double)q[3] * t.h) / S;
    return fmin(o[2] - o[0], o[3] - o[1]) > 0.01;
}

__global__ __launch_bounds__(64) void aug_mosaic_kernel(const ct_aug_sample* __restrict__ samples, int num_images,
                                                        int max_gt, unsigned long long seed, int S, int margin,
                                                        AugPlan* __restrict__ plans, ct_mosaic_tile* __restrict__ tiles,
                                                        ct_aug_sample* __restrict__ fixed, int* __restrict__ counts,
                                                        float* rows)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= num_images) return;
    const Words d = philox(seed, samples[4 * i].sample_id, SLOT_MOSAIC, 0);
    const int span = S - 2 * margin + 1;
    const int cx = margin + randrange(span, d.w[0]), cy = margin + randrange(span, d.w[1]);
    int cnt = 0;
    if (lane < 4) {
        const int s = 4 * i + lane;
        ct_aug_sample sm = samples[s];
        cnt = counts[s];
        if (sm.image != i) {                        // refused here; H < 1, W < 1 were refused by the plan launch
            AugPlan p = plans[s];
            identity_plan(p, p.H, p.W);
            plans[s] = p;
            cnt = -1;
        }
        sm.image = i;
        fixed[s] = sm;
        ct_mosaic_tile t;
        t.x0 = (lane & 1) ? cx : 0; t.y0 = (lane & 2) ? cy : 0;
        t.w = (lane & 1) ? S - cx : cx; t.h = (lane & 2) ? S - cy : cy;
        tiles[s] = t;
    }
    ct_mosaic_tile tile[4];
    int n[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tile[k].x0 = (k & 1) ? cx : 0; tile[k].y0 = (k & 2) ? cy : 0;
        tile[k].w = (k & 1) ? S - cx : cx; tile[k].h = (k & 2) ? S - cy : cy;
        n[k] = min(max(__shfl(cnt, k), 0), max_gt);
    }
    // pass 1: does any mapped row of the image pass the filter
    bool any_kept = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* src = rows + (size_t)(4 * i + k) * max_gt * 6;
        for (int base = 0; base < n[k]; base += 64) {
            const int j = base + lane;
            double o[4];
            any_kept |= __ballot(j < n[k] && mosaic_row(src + (size_t)j * 6, tile[k], S, o)) != 0;
        }
    }
    // pass 2: map, filter and compact in place.  A row moves to an index no larger than its own, and every lane of a
    // stride has read its row before any lane writes (the stores depend on the wave's loads), so no row is lost.
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float* slot = rows + (size_t)(4 * i + k) * max_gt * 6;
        int at = 0;
        for (int base = 0; base < n[k]; base += 64) {
            const int j = base + lane;
            double o[4];
            float label = 0.f, weight = 0.f;
            bool keep = false;
            if (j < n[k]) {
                const float* q = slot + (size_t)j * 6;
                keep = mosaic_row(q, tile[k], S, o) || !any_kept;
                label = q[4]; weight = q[5];
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) {
                float* q = slot + (size_t)(at + __popcll(mask & ((1ull << lane) - 1ull))) * 6;
                q[0] = (float)o[0]; q[1] = (float)o[1]; q[2] = (float)o[2]; q[3] = (float)o[3];
                q[4] = label; q[5] = weight;
            }
            at += __popcll(mask);
        }
        if (lane == k) cnt = cnt < 0 ? -1 : at;
    }
    if (lane < 4) counts[4 * i + lane] = cnt;
}

size_t counts_bytes(int num_samples) { return ctdet::align_up((size_t)num_samples * sizeof(int), 256); }
size_t fixed_bytes(int num_samples) { return ctdet::align_up((size_t)num_samples * sizeof(ct_aug_sample), 256); }

// What ct_aug_plan and ct_aug_plan_mosaic (num_samples = 4 * num_images) are handed alike, and what they do alike with it.
struct PlanCall {
    const char* who;                // the entry's name, as its messages spell it
    const ct_aug_sample* samples;
    int num_samples;
    const float* boxes;
    int total_boxes, num_images, max_gt;
    unsigned long long seed;
    float p_expand;
    const int* interp_of_draw5;
    const float* fill3;
    AugPlan* plans;
    float* truths;
    int truths_cap;
    int* gt_off;
    int* status;
    int* counts;                    // the two parts of the workspace both entries have
    float* rows;
    hipStream_t st;
};

// `tiles`: ct_aug_plan_mosaic's extra output; any non-null pointer for ct_aug_plan
int check_pointers(const PlanCall& c, const void* tiles, const void* workspace)
{
    CT_REQUIRE(c.samples && c.interp_of_draw5 && c.fill3 && c.plans && tiles && c.truths && c.gt_off && c.status && workspace,
               "%s: null pointer", c.who);
    CT_REQUIRE(c.boxes || c.total_boxes == 0, "%s: boxes is null with total_boxes=%d", c.who, c.total_boxes);
    return CT_OK;
}

// `product`: how the entry's message names num_samples * max_gt
int check_sizes(const PlanCall& c, const char* product, size_t need, size_t workspace_bytes)
{
    CT_REQUIRE((size_t)c.num_samples * c.max_gt <= (size_t)1 << 28, "%s: %s = %zu is too large", c.who, product,
               (size_t)c.num_samples * c.max_gt);
    CT_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", c.who, workspace_bytes, need);
    return CT_OK;
}

int launch_plan(const PlanCall& c)
{
    Interp5 ip;
    for (int i = 0; i < 5; ++i) ip.v[i] = c.interp_of_draw5[i];
    Fill3 fl;
    for (int i = 0; i < 3; ++i) fl.v[i] = c.fill3[i];
    CT_PROF("aug_plan_kernel", c.st);
    hipLaunchKernelGGL(aug_plan_kernel, dim3(c.num_samples), dim3(64), 0, c.st, c.samples, c.num_samples, c.boxes,
                       c.total_boxes, c.num_images, c.max_gt, c.seed, (double)c.p_expand, ip, fl, c.plans, c.counts, c.rows);
    CT_LAUNCH_CHECK("aug_plan_kernel");
    return CT_OK;
}

// `samples`: the table whose image fields the scan trusts (the caller's, or the mosaic kernel's corrected copy)
int launch_pack(const PlanCall& c, const ct_aug_sample* samples)
{
    CT_PROF("aug_pack_kernel", c.st);
    hipLaunchKernelGGL(aug_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, c.st, samples, c.num_samples, c.num_images, c.max_gt,
                       c.plans, (const int*)c.counts, (const float*)c.rows, c.truths, c.truths_cap, c.gt_off, c.status);
    CT_LAUNCH_CHECK("aug_pack_kernel");
    return CT_OK;
}

}  // namespace

extern "C" size_t ct_aug_plan_workspace_bytes(int num_samples, int max_gt)
{
    if (num_samples < 1 || max_gt < 1) return 0;
    return counts_bytes(num_samples) + (size_t)num_samples * max_gt * 6 * sizeof(float);
}

extern "C" int ct_aug_plan(const ct_aug_sample* samples, int num_samples, const float* boxes, int total_boxes,
                           int num_images, int max_gt, unsigned long long seed, float p_expand,
                           const int* interp_of_draw5, const float* fill3, void* plans_out, float* truths_out,
                           int truths_cap, int* gt_off_out, int* status, void* workspace, size_t workspace_bytes,
                           ct_stream_t stream)
{
    PlanCall c{"ct_aug_plan", samples, num_samples, boxes, total_boxes, num_images, max_gt, seed, p_expand, interp_of_draw5,
               fill3, (AugPlan*)plans_out, truths_out, truths_cap, gt_off_out, status, (int*)workspace, nullptr,
               ctdet::as_stream(stream)};
    if (int e = check_pointers(c, workspace, workspace)) return e;
    CT_REQUIRE(num_samples >= 1 && total_boxes >= 0 && num_images >= 1 && max_gt >= 1 && truths_cap >= 0,
               "ct_aug_plan: num_samples=%d total_boxes=%d num_images=%d max_gt=%d truths_cap=%d", num_samples,
               total_boxes, num_images, max_gt, truths_cap);
    if (int e = check_sizes(c, "num_samples * max_gt", ct_aug_plan_workspace_bytes(num_samples, max_gt), workspace_bytes))
        return e;
    c.rows = (float*)((char*)workspace + counts_bytes(num_samples));
    if (int e = launch_plan(c)) return e;
    return launch_pack(c, samples);
}

extern "C" size_t ct_aug_plan_mosaic_workspace_bytes(int num_images, int max_gt)
{
    if (num_images < 1 || max_gt < 1 || num_images > (1 << 26)) return 0;
    const int num_samples = 4 * num_images;
    return counts_bytes(num_samples) + fixed_bytes(num_samples) + (size_t)num_samples * max_gt * 6 * sizeof(float);
}

extern "C" int ct_aug_plan_mosaic(const ct_aug_sample* samples, int num_images, const float* boxes, int total_boxes,
                                  int max_gt, unsigned long long seed, float p_expand, const int* interp_of_draw5,
                                  const float* fill3, int size, int margin, void* plans_out, ct_mosaic_tile* tiles_out,
                                  float* truths_out, int truths_cap, int* gt_off_out, int* status, void* workspace,
                                  size_t workspace_bytes, ct_stream_t stream)
{
    PlanCall c{"ct_aug_plan_mosaic", samples, 0, boxes, total_boxes, num_images, max_gt, seed, p_expand, interp_of_draw5,
               fill3, (AugPlan*)plans_out, truths_out, truths_cap, gt_off_out, status, (int*)workspace, nullptr,
               ctdet::as_stream(stream)};
    if (int e = check_pointers(c, tiles_out, workspace)) return e;
    CT_REQUIRE(num_images >= 1 && num_images <= (1 << 26) && total_boxes >= 0 && max_gt >= 1 && truths_cap >= 0,
               "ct_aug_plan_mosaic: num_images=%d total_boxes=%d max_gt=%d truths_cap=%d", num_images, total_boxes, max_gt,
               truths_cap);
    CT_REQUIRE(size >= 2 && size <= 4096, "ct_aug_plan_mosaic: size=%d", size);
    CT_REQUIRE(margin >= 1 && margin <= size / 2, "ct_aug_plan_mosaic: margin=%d outside 1..%d", margin, size / 2);
    c.num_samples = 4 * num_images;
    if (int e = check_sizes(c, "4 * num_images * max_gt", ct_aug_plan_mosaic_workspace_bytes(num_images, max_gt),
                            workspace_bytes))
        return e;
    CT_REQUIRE(((size_t)workspace & 15) == 0, "ct_aug_plan_mosaic: workspace is not 16-byte aligned");
    ct_aug_sample* fixed = (ct_aug_sample*)((char*)workspace + counts_bytes(c.num_samples));
    c.rows = (float*)((char*)fixed + fixed_bytes(c.num_samples));
    if (int e = launch_plan(c)) return e;
    {
        CT_PROF("aug_mosaic_kernel", c.st);
        hipLaunchKernelGGL(aug_mosaic_kernel, dim3(num_images), dim3(64), 0, c.st, samples, num_images, max_gt, seed, size,
                           margin, c.plans, tiles_out, fixed, c.counts, c.rows);
        CT_LAUNCH_CHECK("aug_mosaic_kernel");
    }
    return launch_pack(c, fixed);
}
