/* ctdet.h -- C ABI of libctdet.so: the MI355X (gfx950) detection hot path of
 * Ze-Yang/Context-Transformer (RFBNet-VGG forward, Context-Transformer attention,
 * prior-box decode / IoU matching, NMS), hand-written HIP behind plain pointers.
 *
 * Conventions
 *   - every entry point returns an int status (CT_OK == 0); ct_last_error_string()
 *     gives the text of the last failure on the calling thread;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); device
 *     entry points are asynchronous on it and never allocate: scratch memory comes
 *     from the caller through the matching ct_*_workspace_bytes() query;
 *   - all tensors are contiguous fp32 unless stated; "dev" = device pointer,
 *     "host" = host pointer; int = int32;
 *   - no torch / C++ types cross this boundary.
 *
 * Each declaration cites the reference interface it replaces (paths relative to the
 * reference repository).  The reference's only native symbol is `_nms`
 * (utils/nms/gpu_nms.hpp:1-2); everything else is stock PyTorch/ATen called from
 * Python, so for those the cited "interface" is the Python call site.
 */
#ifndef CTDET_H
#define CTDET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTDET_ABI_VERSION 1

enum {
    CT_OK = 0,
    CT_ERR_INVALID = 1,     /* bad argument / unsupported geometry            */
    CT_ERR_HIP = 2,         /* a HIP runtime call or kernel launch failed     */
    CT_ERR_WORKSPACE = 3,   /* caller-provided workspace too small            */
    CT_ERR_UNSUPPORTED = 4  /* valid request this build does not implement    */
};

typedef void* ct_stream_t;

int ct_abi_version(void);
const char* ct_last_error_string(void);
/* arch: e.g. "gfx950"; any out pointer may be NULL. */
int ct_device_info(int device, int* cu_count, int* lds_bytes_per_cu, char* arch, int arch_len);

/* Training scratch zeroing.  The accumulating training kernels (BatchNorm statistics / backward reductions, bias
 * gradients, split weight gradients, the Winograd weight-gradient workspace) zero their accumulation buffer with one
 * small memset per launch (~150 per training step).  ct_scratch_prezeroed(1) (per calling thread) makes the caller
 * responsible instead: ctdet/train_engine.py keeps those buffers in three arenas and zeroes each with ONE memset per
 * pass.  ct_scratch_prezeroed(0) restores the default. */
int ct_scratch_prezeroed(int on);

/* Batched weight packing for training steps (every optimizer step changes every weight, and each fused conv needs
 * its forward AND its data-gradient layout re-packed: ~130 small launches per step).  Between
 * ct_pack_record_begin() and ct_pack_record_end() the ct_conv_pack_weights* entry points called on THIS thread
 * record their arguments instead of launching; _end copies the table to caller memory (ct_pack_record_bytes());
 * ct_pack_run() then re-packs everything recorded in two launches.  The table holds the weight and output
 * pointers: record again when a parameter is re-allocated. */
int ct_pack_record_begin(void);
size_t ct_pack_record_bytes(void);
int ct_pack_record_end(void* table_dev, size_t table_bytes, int* num_direct, int* num_wino, ct_stream_t stream);
int ct_pack_run(const void* table_dev, int num_direct, int num_wino, ct_stream_t stream);

/* Measurement aid (bench.py `roofline.stages`): while enabled, the post-processing, score-fusion and attention
 * entry points bracket each of their kernel launches with HIP events on the launch stream.
 * ct_profile_enable(on) clears the records; ct_profile_collect waits for the recorded events and returns
 * (kernel name, milliseconds) per launch in launch order; *num_records = records available (may exceed max). */
typedef struct ct_profile_record {
    const char* name;   /* static string owned by the library */
    float ms;
} ct_profile_record;
int ct_profile_enable(int on);
int ct_profile_collect(ct_profile_record* out, int max_records, int* num_records);

/* ------------------------------------------------------------------ NMS ---- */

/* Drop-in for the reference's only native symbol:
 *   void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num,
 *             int boxes_dim, float nms_overlap_thresh, int device_id);
 *   (utils/nms/gpu_nms.hpp:1-2, utils/nms/nms_kernel.cu:91-144; caller utils/nms/gpu_nms.pyx:29)
 * Same contract: host buffers owned by the caller, boxes already sorted by descending
 * score, row = [x1,y1,x2,y2,score,...] (boxes_dim >= 4 floats per row), +1 pixel
 * convention, suppress IoU > thresh, keep_out = ascending indices into the sorted array.
 * Differences: returns a status instead of printing CUDA errors; does not change the
 * process-global current device (it is restored); the temporary device buffer is kept per thread between calls
 * (grown on demand) instead of being allocated and freed every time. */
int ct_nms_sorted_host(int* keep_out, int* num_out, const float* boxes_host, int boxes_num,
                       int boxes_dim, float nms_overlap_thresh, int device_id);
/* NMS mode flags (the `mode` / `ge` argument of the NMS entry points). */
#define CT_NMS_GT 0     /* suppress IoU >  thresh, +1 pixel convention (utils/nms/nms_kernel.cu:24-32,71) */
#define CT_NMS_GE 1     /* suppress IoU >= thresh                      (utils/nms/cpu_nms.pyx:65)          */
#define CT_NMS_PLAIN 2  /* no +1, union = (area_j - inter) + area_i    (utils/box_utils.py:238-302 `nms`)  */
/* Same with the rule selectable: mode = CT_NMS_GT | CT_NMS_GE, optionally | CT_NMS_PLAIN. */
int ct_nms_sorted_host_mode(int* keep_out, int* num_out, const float* boxes_host, int boxes_num,
                            int boxes_dim, float nms_overlap_thresh, int mode, int device_id);

/* Batched device NMS over independent segments (one per (image, class) of test.py:142-153).
 *   dets      dev [total,5]  rows [x1,y1,x2,y2,score], each segment sorted by descending score
 *   seg_off   dev [S+1]      segment s = rows seg_off[s] .. seg_off[s+1]-1
 *   keep      dev [total]    out: for segment s, keep[seg_off[s] + i], i < keep_count[s], are
 *                            the kept row positions RELATIVE to the segment, ascending
 *   keep_count dev [S]
 * max_seg_len bounds every segment length (sizes the launch). */
size_t ct_nms_batched_workspace_bytes(int total_boxes, int num_segments);
int ct_nms_batched_dev(const float* dets, const int* seg_off, int num_segments, int max_seg_len,
                       float thresh, int ge, int* keep, int* keep_count,
                       void* workspace, size_t workspace_bytes, ct_stream_t stream);

/* CPU NMS of the reference's `--cpu` path: utils/nms/cpu_nms.pyx:17-68 (`cpu_nms`).
 * dets host [n,5] UNSORTED; keep_out host [n] receives original indices in descending
 * score order (ties: lower index first); suppress IoU >= thresh (ge=1) or > (ge=0). */
int ct_cpu_nms(const float* dets_host, int n, float thresh, int ge, int* keep_out, int* num_out);
/* utils/nms/cpu_nms.pyx:70-163 (`cpu_soft_nms`): mutates boxes [n,5] in place, *n_out = N'. */
int ct_cpu_soft_nms(float* boxes_host, int n, float sigma, float Nt, float threshold,
                    unsigned method, int* n_out);

/* Soft-NMS on the device (the device form of `cpu_soft_nms`), one workgroup per segment.  Segments as for
 * ct_nms_batched_dev: dets dev [total,5], each segment in descending score order (lower prior index first on ties).
 *   method 0 hard (ov > Nt removes), 1 linear (score *= 1 - ov when ov > Nt), 2 Gaussian (score *= exp(-ov^2 / sigma));
 *   a row whose decayed score falls below score_threshold is removed (reference default 0.001);
 *   max_emit > 0: a segment stops after max_emit rows, except for further rows that tie with the last one; 0: no limit.
 *   out_rows  dev [total,5]  out_rows[seg_off[s] + i], i < out_count[s]: the emitted rows (box, decayed score) in
 *                            emission order = non-increasing score
 *   out_pos   dev [total]    position of each emitted row relative to its segment
 *   out_count dev [S]        rows emitted; -1: the workspace does not cover segment s (queried with too few rows)
 * Nothing is written past out_count[s] rows of a segment.  Methods 0 and 1 equal ct_cpu_soft_nms bit for bit on tie-free
 * input; method 2 makes the same decisions with scores within an ulp of the weight per decay (the double-precision exp is
 * another libm's).  Segments of at most ct_soft_nms_lds_rows() rows keep their state in LDS, longer ones in the workspace. */
int ct_soft_nms_lds_rows(void);
size_t ct_soft_nms_batched_workspace_bytes(int total_rows, int num_segments);
int ct_soft_nms_batched_dev(const float* dets, const int* seg_off, int num_segments, int max_seg_len,
                            int method, float sigma, float Nt, float score_threshold, int max_emit,
                            float* out_rows, int* out_pos, int* out_count,
                            void* workspace, size_t workspace_bytes, ct_stream_t stream);

/* Matrix NMS (Wang et al., SOLOv2 section 3.3) on the device, one workgroup per segment: every row's score decay in closed
 * form from the pairwise IoUs of the sorted rows, corrected by how much each suppressor was itself suppressed.  Segments as
 * for ct_soft_nms_batched_dev (descending score, lower prior index first on ties).  On one segment:
 *   1. only the first n = min(len, pre_top) rows take part, rows at sorted positions >= pre_top are dropped (`nms_pre`);
 *      0 < pre_top <= ct_matrix_nms_max_rows() (at least 1024: what the kernel's LDS layout holds);
 *   2. ov(i, j), i < j: the +1 pixel fp32 expression of ct_soft_nms_batched_dev and ct_cpu_soft_nms (iw = min(x2) - max(x1)
 *      + 1, ih likewise, ov = 0 unless iw > 0 && ih > 0, ua = area_i + area_j - iw * ih, ov = iw * ih / ua; IEEE division,
 *      no contraction);
 *   3. cmax[i] = max over k < i of ov(k, i), cmax[0] = 0;
 *   4. decay[j] = min(1, min over i < j of t(i, j)), decay[0] = 1, with
 *        method 1 (linear)    t = (1 - ov(i,j)) / (1 - cmax[i]) in fp32, IEEE quotient; a term whose denominator is 0 is
 *                             skipped: a row that exactly duplicates an earlier one is itself decayed to 0 and suppresses
 *                             nothing;
 *        method 2 (Gaussian)  t = (float)exp(((double)cmax[i]^2 - (double)ov(i,j)^2) / (double)sigma) -- sigma divides, as in
 *                             the soft-NMS entries: sigma = 0.5 here is the papers' sigma = 2;
 *   5. score'[j] = score[j] * decay[j] (one fp32 multiply); a row with score' < score_threshold (>= 0) is removed;
 *   6. emission in non-increasing score', ties lower sorted position first;
 *   7. max_emit > 0: a segment stops after max_emit rows, except for further rows that tie with the last one; 0: no limit.
 * There is no Nt.  out_rows / out_pos / out_count as for ct_soft_nms_batched_dev (out_pos: sorted positions relative to
 * the segment; out_count is never -1).  dets is not modified, nothing is written past out_count[s] rows of a segment, an
 * empty segment gives 0.  The workspace query returns 0 and workspace may be NULL: a segment's state lives in LDS.
 * Minima and maxima do not depend on the order they are taken in: method 1 equals ct_cpu_matrix_nms bit for bit.  Method 2
 * differs from it only by the two libms' double exp rounded to fp32, at most one fp32 ulp of decay, plus the product's
 * rounding: every score is within 2^-22 of the host's, relatively, and decisions and order are the same wherever the
 * host's own margins (between consecutive emitted scores, and to score_threshold) exceed that. */
int ct_matrix_nms_max_rows(void);
size_t ct_matrix_nms_batched_workspace_bytes(int total_rows, int num_segments);
int ct_matrix_nms_batched_dev(const float* dets, const int* seg_off, int num_segments, int max_seg_len,
                              int method, float sigma, float score_threshold, int pre_top, int max_emit,
                              float* out_rows, int* out_pos, int* out_count,
                              void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* Host twin on one segment: rows_sorted host [n,5] in the pipeline's order -> out_rows host [n,5], out_pos host [n] (what
 * the device entry emits for that segment), *n_out rows.  The rule above as plain loops; any pre_top > 0. */
int ct_cpu_matrix_nms(const float* rows_sorted, int n, int method, float sigma, float score_threshold, int pre_top,
                      int max_emit, float* out_rows, int* out_pos, int* n_out);

/* ----------------------------------------------------- boxes / detection ---- */

/* utils/box_utils.py:184-202 `decode(loc, priors, variances)`, batched over images:
 * loc dev [B,P,4], priors dev [P,4] (cx,cy,w,h) -> boxes dev [B,P,4] (x1,y1,x2,y2),
 * each coordinate multiplied by scale4[c] if scale4 != NULL (dev [4] or per image [B,4],
 * `boxes *= scale` of test.py:136). */
int ct_decode(const float* loc, const float* priors, int batch, int num_priors,
              float var0, float var1, const float* scale4, int scale_per_image,
              float* boxes, ct_stream_t stream);
/* utils/box_utils.py:135-156 `encode(matched, priors, variances)`: [P,4],[P,4] -> [P,4]. */
int ct_encode(const float* matched, const float* priors, int num_priors, float var0, float var1,
              float* out, ct_stream_t stream);
/* layers/functions/detection.py:18-55 `Detect.forward`: decode + score fusion
 * scores[b,p,0] = obj[b,p,0]; scores[b,p,1+k] = obj[b,p,1]*conf[b,p,k].
 * If apply_softmax != 0, conf/obj are raw logits and the eval-time softmaxes of
 * models/RFB_Net_vgg.py:279-285 are fused in.  scale4 (dev [4] or [B,4], may be NULL) fuses
 * the `boxes *= scale` of test.py:136. */
int ct_detect_fused(const float* loc, const float* conf, const float* obj, const float* priors,
                    int batch, int num_priors, int num_fg, float var0, float var1,
                    int apply_softmax, const float* scale4, int scale_per_image,
                    float* boxes, float* scores, ct_stream_t stream);
/* torch.nn.functional.softmax(x, dim=-1) of models/RFB_Net_vgg.py:282-284: [rows, cols]. */
int ct_softmax_lastdim(const float* in, float* out, long rows, int cols, ct_stream_t stream);

/* utils/box_utils.py:50-68 `jaccard(box_a, box_b)`: a dev [A,4], b dev [Bn,4] point form
 * -> out dev [A,Bn]; no +1 convention. b_center_form != 0: b is (cx,cy,w,h) and
 * point_form (utils/box_utils.py:5-14) is applied on the fly. */
int ct_jaccard(const float* a, int na, const float* b, int nb, int b_center_form,
               float* out, ct_stream_t stream);

/* utils/box_utils.py:83-132 `match(...)` for a whole batch (the Python loop of
 * layers/modules/multibox_loss_combined.py:70-74):
 *   truths dev [sum G,6] rows [x1,y1,x2,y2,label,weight]; gt_off dev [B+1]
 *   priors dev [P,4] center form
 *   -> loc_t [B,P,4], conf_t [B,P,2] (label, weight), obj_t uint8 [B,P], overlap [B,P] or NULL
 * Force-match collisions keep the reference's "later GT wins" order (:122-123).
 * max_gt = the largest per-image box count in gt_off (any size); the workspace has max_gt slots per image, and an
 * image with MORE boxes than max_gt is matched against its first max_gt boxes only (never an out-of-bounds write). */
size_t ct_match_workspace_bytes(int batch, int num_priors, int max_gt);
int ct_match_batched(const float* truths, const int* gt_off, int batch, int max_gt,
                     const float* priors, int num_priors, float threshold, float var0, float var1,
                     float* loc_t, float* conf_t, uint8_t* obj_t, float* overlap,
                     void* workspace, size_t workspace_bytes, ct_stream_t stream);

/* ADAPTIVE TRAINING SAMPLE SELECTION (ATSS, Zhang et al., CVPR 2020): the second matcher.  It replaces the hand-set IoU
 * threshold of ct_match_batched by one computed per box from the box's own candidates; the outputs have the same layout, so
 * the loss entries below read either matcher's result.
 *
 * Inputs are those of ct_match_batched, plus two new ones:
 *   truths dev [sum G,6], gt_off dev [B+1], priors dev [P,4] in centre form.
 *   level_off: a HOST array of L+1 ascending prior offsets, with level_off[0] = 0 and level_off[L] = P.  It gives the pyramid
 *     level of every prior.
 *   topk.
 * All fp32 arithmetic is rounded operation by operation (no FMA contraction).
 *
 * For every image b, every box g < min(G_b, max_gt) is handled independently of the others.  The max_gt truncation contract of
 * ct_match_batched is kept.
 *  1. DEGENERATE BOXES.  A box with !(x2 > x1 && y2 > y1) is skipped: it has no candidates and no positives.
 *     (ct_match_batched does not skip such boxes and can write logf(0) for them.  Here the result stays finite.)
 *  2. CANDIDATES.  The box centre is gx = (x1+x2)/2, gy = (y1+y2)/2.  The distance to prior p is d = dx*dx + dy*dy, with
 *     dx = pcx - gx and dy = pcy - gy.  In each level l the candidates are the min(topk, n_l) priors with the smallest d.  Ties
 *     go to the lower prior index.  Candidate order is level-major, then ascending (d, index).  The priors of one cell share a
 *     centre: with topk = 9 and 6 priors per cell this takes the nearest cell's six priors and three of the next cell, which
 *     is the behaviour of the published implementations.
 *  3. IOU.  The IoU of each candidate is the expression of ct_jaccard with b_center_form != 0: inter / (area_a + area_b -
 *     inter) of the box and the prior in point form.
 *  4. THRESHOLD.  Let n be the number of candidates.  mean is the sum of the IoUs, accumulated in float64 in candidate order,
 *     divided by n.  var is the float64 sum of (iou - mean)^2, in the same order, divided by n - 1.  It is 0 when n < 2.
 *     t = (float)(mean + sqrt(var)).
 *  5. POSITIVE CANDIDATES.  A candidate is positive if iou >= t and x1 < pcx < x2 and y1 < pcy < y2.  The inequalities are
 *     strict and are taken on the fp32 values as they are.
 *  6. FORCED POSITIVE.  If no candidate of a non-degenerate box is positive, the candidate with the largest IoU becomes its one
 *     forced positive.  The first in candidate order wins a tie.  The centre test is waived for it.  This keeps the reference
 *     matcher's property that every box trains at least one prior, which a few-shot detector cannot give up; it is the one
 *     deliberate departure from the published rule.  A BOX CAN STILL END WITH NO PRIOR if all of its positives are lost under
 *     rule 7.
 *  7. CONFLICTS.  A prior claimed by several boxes goes to the claim that wins this order: a forced claim over an ordinary
 *     one, then the larger IoU, then the lower box index.
 *  8. OUTPUTS.  The layout is ct_match_batched's.  An assigned prior gets loc_t = the encode expression of ct_encode /
 *     ct_match_batched, conf_t = (label, weight) of its box, label -1 and mixup weights included, and obj_t = label != 0.
 *     Every other prior gets loc_t = 0, conf_t = (0, 1) and obj_t = 0, exactly.  overlap may be NULL: it holds the IoU with
 *     the assigned box, else 0.  gt_stats may be NULL: it is [B, max_gt, 4] floats = (t, number of candidates, number of
 *     positive candidates before conflicts with the forced one counted, forced ? 1 : 0); rows of skipped or absent boxes are
 *     zeros.
 * An image's result never depends on its batch mates, and the same inputs give the same bits on every run (conflicts are
 * resolved by an order-independent packed atomicMax).  The entry makes no allocation, does no host synchronisation and makes
 * no H2D copy: level_off travels in the kernel arguments.  One memset and two launches on `stream`.
 * workspace: ct_atss_workspace_bytes(batch, num_priors, max_gt) bytes, 8-byte aligned.
 * CT_ERR_INVALID before any HIP call: NULL tensors (overlap and gt_stats excepted) or a NULL level_off; batch, num_priors or
 * max_gt < 1; num_priors above 2^30 or batch above 65535; num_levels outside 1..8; topk outside 1..16; a level_off that is
 * not 0 = off[0] < ... < off[L] = P; a variance that is not positive and finite; a workspace that is too small or not
 * 8-byte aligned. */
size_t ct_atss_workspace_bytes(int batch, int num_priors, int max_gt);
int ct_atss_match_batched(const float* truths, const int* gt_off, int batch, int max_gt,
                          const float* priors, int num_priors, const int* level_off_host, int num_levels,
                          int topk, float var0, float var1, float* loc_t, float* conf_t, uint8_t* obj_t,
                          float* overlap, float* gt_stats, void* workspace, size_t workspace_bytes,
                          ct_stream_t stream);

/* TASK-ALIGNED ASSIGNMENT (TAL; Feng et al., TOOD, ICCV 2021; the family of SimOTA): the prediction-aware matcher.  Where
 * ct_match_batched and ct_atss_match_batched read the ground truth and the priors only, this one ranks the priors inside a
 * box by how well the network currently classifies and localises from them, m = score^alpha * IoU(predicted box, box)^beta,
 * and trains the best topk.  The outputs have the layout of the other two, so the loss entries below read any matcher's result.
 *
 * truths, gt_off, priors, max_gt (truncation contract included), loc_t, conf_t, obj_t and overlap are those of
 * ct_atss_match_batched.  pred_boxes dev [B,P,4] (point form) and pred_scores dev [B,P,score_cols] are in the layout
 * ct_detect_fused writes: column 0 is the background / objectness-negative probability, column c >= 1 is foreground class c,
 * score_cols = 1 + num_fg.  alpha2 = 2 * alpha (0..4, so alpha is 0, 0.5, 1, 1.5 or 2); beta is an integer 0..8.
 * All fp32 arithmetic is rounded operation by operation (no FMA contraction; IEEE division and square root).
 *
 * For every image b, every box g < min(G_b, max_gt) is handled independently of the others.
 *  1. DEGENERATE BOXES.  A box with !(x2 > x1 && y2 > y1) is skipped: it has no candidates and no positives.
 *  2. CANDIDATES.  The priors whose centre lies strictly inside the box: x1 < pcx < x2 && y1 < pcy < y2, on the fp32 values as
 *     they are.
 *  3. METRIC.  For a candidate p: u = the IoU expression of ct_jaccard of the box and pred_boxes[b,p], and u = 0 if !(u > 0)
 *     (NaN and Inf-born boxes included).  s = pred_scores[b,p,L] if the box's label L is an integer in 1..score_cols-1;
 *     otherwise (label -1, 0 or out of range) s = 1.f - pred_scores[b,p,0]; s = 0 if !(s > 0).  m = s^(alpha2/2) * u^beta in
 *     fp32, in this order: start from 1.f, multiply by sqrtf(s) if alpha2 is odd, then by s alpha2/2 times, then by u beta
 *     times.  Finally m = 0 if !(m >= FLT_MIN): the result is the same whether or not fp32 subnormals are flushed (products
 *     of values <= 1 only shrink).  A candidate is ELIGIBLE if m > 0.
 *  4. POSITIVES.  The min(topk, eligible) eligible candidates with the largest m.  Ties go to the lower prior index.
 *  5. FORCED POSITIVE.  A non-degenerate box with no eligible candidate (no centre inside, or every metric 0) takes one forced
 *     positive: the prior with the largest IoU of the box and the prior in point form, over ALL priors, lowest index on a
 *     tie.  Its claim carries that IoU.  As in ATSS, every box trains at least one prior unless rule 6 takes it away.
 *  6. CONFLICTS.  A prior claimed by several boxes goes to the claim that wins this order: a forced claim over an ordinary
 *     one, then the larger u (for a forced claim, its prior IoU), then the lower box index.
 *  7. OUTPUTS.  An assigned prior gets loc_t = the encode expression of ct_encode, conf_t = (label, weight) of its box and
 *     obj_t = label != 0.  Every other prior gets loc_t = 0, conf_t = (0, 1) and obj_t = 0, exactly.  overlap may be NULL: it
 *     holds the winning claim's u, else 0.  gt_stats may be NULL: it is [B, max_gt, 4] floats = (eligible count, number of
 *     positives before conflicts with the forced one counted, m of the last positive chosen or 0 if forced, forced ? 1 : 0);
 *     rows of skipped or absent boxes are zeros.
 * An image's result never depends on its batch mates, and the same inputs give the same bits on every run.  The entry makes
 * no allocation, does no host synchronisation and makes no H2D copy.  One memset and two launches on `stream`.  The selection
 * kernel evaluates a candidate (its predicted box, score and metric) once while it scans and once more if it is chosen; its
 * LDS key buffer holds ct_tal_lds_keys() keys whatever P is, and is reduced to the topk best whenever it could overflow.
 * workspace: ct_tal_workspace_bytes(batch, num_priors, max_gt) bytes, 8-byte aligned.
 * CT_ERR_INVALID before any HIP call: NULL tensors (overlap and gt_stats excepted); batch, num_priors or max_gt < 1;
 * num_priors above 2^30 or batch above 65535; score_cols < 2; topk outside 1..16; alpha2 outside 0..4; beta outside 0..8; a
 * variance that is not positive and finite; a workspace that is too small or not 8-byte aligned. */
int ct_tal_lds_keys(void);
size_t ct_tal_workspace_bytes(int batch, int num_priors, int max_gt);
int ct_tal_match_batched(const float* truths, const int* gt_off, int batch, int max_gt,
                         const float* priors, int num_priors,
                         const float* pred_boxes  /* dev [B,P,4] point form */,
                         const float* pred_scores /* dev [B,P,score_cols] */, int score_cols,
                         int topk, int alpha2, int beta, float var0, float var1,
                         float* loc_t, float* conf_t, uint8_t* obj_t,
                         float* overlap /* or NULL */, float* gt_stats /* or NULL */,
                         void* workspace, size_t workspace_bytes, ct_stream_t stream);

/* layers/modules/multibox_loss_combined.py:76-122 (`MultiBoxLoss_combined.forward` after the matching): the loss
 * arithmetic, fused.  Forward = three launches, backward = one; no allocation, no host synchronisation, capturable.
 *   loc dev [B,P,4], conf dev [B,P,C-1], obj dev [B,P,2]      the network's raw outputs (C = num_classes >= 2)
 *   loc_t [B,P,4], conf_t [B,P,2] (label, mixup weight), obj_t uint8 [B,P]      as ct_match_batched writes them
 *   -> sums dev [3] = (sum loc, sum cls, sum obj) UN-normalised (the caller divides by n or by its data-parallel
 *      normaliser), num_pos dev int64 [B], n dev int64 [1] = sum of num_pos, w dev [B,P] = weight * (pos | neg),
 *      the per-prior loss weight the backward reads.
 * num_pos rule (:76-77): long(sum of weight over priors with label > 0); the sum is accumulated in fp64 in a fixed
 * order, rounded once to fp32 and truncated, so it does not depend on launch geometry.
 * Hard negatives (:88-96): num_neg = min(negpos_ratio * num_pos, P - 1) priors with the largest objectness loss (0
 * where obj_t is set).  Tie rule: priors above the num_neg-th largest loss are drawn; priors EQUAL to it are drawn in
 * ascending prior index until num_neg is reached (what a stable descending sort gives), zero-loss priors included.
 * Label -1 (ignored box) rows are evaluated against class 0 and carry weight 0; the background logit is
 * obj0 + logsumexp(conf).  Bit-reproducible from run to run; an image's selection never depends on its batch mates. */
size_t ct_multibox_loss_workspace_bytes(int batch, int num_priors, int num_classes);
int ct_multibox_loss_fwd(const float* loc, const float* conf, const float* obj, const float* loc_t,
                         const float* conf_t, const uint8_t* obj_t, int batch, int num_priors, int num_classes,
                         int negpos_ratio, float* sums, long long* num_pos, long long* n, float* w,
                         void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* Gradients of g[0]*sums[0] + g[1]*sums[1] + g[2]*sums[2] w.r.t. (loc, conf, obj); g dev [3], w from the forward.
 * Every element of dloc / dconf / dobj is written (no memset needed); a row with w = 0 gets exact zeros whatever
 * its logits. */
int ct_multibox_loss_bwd(const float* loc, const float* conf, const float* obj, const float* loc_t,
                         const float* conf_t, const uint8_t* obj_t, const float* w, const float* g,
                         int batch, int num_priors, int num_classes, float* dloc, float* dconf, float* dobj,
                         ct_stream_t stream);

/* The same loss with a choice of localisation term (no counterpart in the reference, whose only term is smooth-L1):
 * loc_loss = CT_LOC_SMOOTH_L1 is ct_multibox_loss_fwd / _bwd launch for launch and bit for bit (priors may be NULL);
 * the IoU kinds replace the smooth-L1 term of every positive row (label > 0) by L below.  Selection, mining, w, num_pos,
 * n, sums[1], sums[2], dconf and dobj do not depend on loc_loss.  Same workspace query, same launch counts.
 *   priors dev [P,4] centre form (pcx, pcy, pw, ph), the priors the matcher encoded loc_t against; var0, var1 its variances.
 * Definition.  D(l, p) is utils/box_utils.py:184 `decode`: cx = pcx + l0 var0 pw, cy = pcy + l1 var0 ph, w = pw exp(l2 var1),
 * h = ph exp(l3 var1), box (cx - w/2, cy - h/2, cx + w/2, cy + h/2).  A = D(loc, p) is the prediction, T = D(loc_t, p) the
 * matched box (it recovers the ground truth up to rounding, and it is the definition here: no new matcher output).
 *   iw = max(0, min(A.x2, T.x2) - max(A.x1, T.x1)), ih likewise; inter = iw ih; union = A.w A.h + T.w T.h - inter;
 *   IoU = inter / union; cw = max(A.x2, T.x2) - min(A.x1, T.x1), ch likewise;
 *   CT_LOC_IOU:  L = 1 - IoU
 *   CT_LOC_GIOU: L = 1 - IoU + (cw ch - union) / (cw ch)
 *   CT_LOC_DIOU: L = 1 - IoU + rho2 / c2,  rho2 = squared distance of the two centres, c2 = cw^2 + ch^2
 *   CT_LOC_CIOU: L = DIoU's + alpha v,  v = (4 / pi^2) (atan(T.w / T.h) - atan(A.w / A.h))^2, alpha = v / ((1 - IoU) + v),
 *                alpha = 0 when v = 0; alpha is a CONSTANT in the backward pass (as in the published implementations).
 * sums[0] = sum over positives of L * weight, in the fixed-order fp64 accumulation of the smooth-L1 term.
 * A row that is not positive, or whose weight is 0, contributes 0 and gets dloc = 0 exactly: its loc, loc_t and prior are not
 * read.  The exponent is not clamped: non-finite inputs on a positive row give non-finite outputs.  At a kink (two equal
 * arguments of a min / max, iw or ih exactly 0) the gradient is one of the one-sided derivatives.
 * CT_ERR_INVALID before any HIP call: an unknown loc_loss, NULL priors with an IoU kind, a variance that is not a
 * positive finite number. */
enum {
    CT_LOC_SMOOTH_L1 = 0,
    CT_LOC_IOU = 1,
    CT_LOC_GIOU = 2,
    CT_LOC_DIOU = 3,
    CT_LOC_CIOU = 4
};
int ct_multibox_loss_fwd_loc(const float* loc, const float* conf, const float* obj, const float* loc_t,
                             const float* conf_t, const uint8_t* obj_t, int batch, int num_priors, int num_classes,
                             int negpos_ratio, float* sums, long long* num_pos, long long* n, float* w,
                             void* workspace, size_t workspace_bytes, ct_stream_t stream,
                             const float* priors, int loc_loss, float var0, float var1);
int ct_multibox_loss_bwd_loc(const float* loc, const float* conf, const float* obj, const float* loc_t,
                             const float* conf_t, const uint8_t* obj_t, const float* w, const float* g,
                             int batch, int num_priors, int num_classes, float* dloc, float* dconf, float* dobj,
                             ct_stream_t stream, const float* priors, int loc_loss, float var0, float var1);

/* The same loss with a choice of classification terms as well, the options in one struct (so this is the last suffix of
 * the argument list).  conf_loss = CT_CONF_CE is the _loc entries launch for launch and bit for bit (focal_gamma and
 * focal_alpha are then not read); CT_CONF_FOCAL replaces the two cross-entropies over the mined sample by focal terms
 * over EVERY prior that is not ignored (no counterpart in the reference).  Same workspace query; forward three launches
 * (the per-image pass holds no keys and runs no radix passes), backward one; no allocation, no host synchronisation,
 * capturable.
 * Definition of CT_CONF_FOCAL.  The matcher's outputs as they are: conf_t = (label, weight), obj_t = label != 0, background
 * rows carry weight 1, ignored rows label -1.  Row weight w = weight when label >= 0, w = 0 for an ignored row; nothing is
 * mined, negpos_ratio is accepted and not read; num_pos, n and the localisation term (any loc_loss) are what they are with
 * CT_CONF_CE.  s = softmax(obj) over the 2 columns, q = softmax(conf) over the C-1 columns; the fused class probabilities
 * are p_0 = s_0, p_k = s_1 q_k.  For a target t with probability p, and m = THE SUM OF THE OTHER PROBABILITIES (never 1 - p):
 *   FL = -a m^gamma log p,   0^0 = 1,   log p taken from the logits (the cross-entropy of CT_CONF_CE, negated)
 *   objectness term: t = obj_t;  a = alpha for t = 1, 1 - alpha for t = 0, and a = 1 when alpha < 0
 *   class term:      t = clamp(label, 0, C-1), p = p_t;  a = alpha for a foreground target, 1 - alpha for background
 *                    (1 when alpha < 0)
 *   sums[1] = sum of w FL_cls, sums[2] = sum of w FL_obj, in the fixed-order fp64 accumulation of the other entries.
 * Gradient: with r = log p / m (r = -1 where m = 0) and c = a m^gamma (1 - gamma p r), dFL/dz_j = c (p_j - [j = t]), finite
 * for every gamma >= 0.  Through the fused logits: d/dconf_k = c ([t >= 1] q_k - [k = t]), d/dobj = c (s - onehot(t >= 1)),
 * and the objectness term adds c_obj (s - onehot(obj_t)).
 * A row with w = 0 gets exact zeros whatever its logits hold, and its logits are not read.  The conf row of a background
 * prior (label 0) is read neither in the forward nor in the backward, and its dconf is exact zeros.  w (output) = the row
 * weight above.
 * CT_ERR_INVALID before any HIP call: NULL terms, what the _loc entries refuse, an unknown conf_loss, and with
 * CT_CONF_FOCAL a focal_gamma that is not finite and >= 0 or a focal_alpha that is neither in [0, 1] nor negative. */
enum {
    CT_CONF_CE = 0,
    CT_CONF_FOCAL = 1
};
typedef struct ct_loss_terms {
    const float* priors;            /* as in the _loc entries; may be NULL with CT_LOC_SMOOTH_L1 */
    int loc_loss;                   /* CT_LOC_* */
    float var0, var1;
    int conf_loss;                  /* CT_CONF_* */
    float focal_gamma, focal_alpha; /* read with CT_CONF_FOCAL only */
} ct_loss_terms;
int ct_multibox_loss_fwd_terms(const float* loc, const float* conf, const float* obj, const float* loc_t,
                               const float* conf_t, const uint8_t* obj_t, int batch, int num_priors, int num_classes,
                               int negpos_ratio, float* sums, long long* num_pos, long long* n, float* w,
                               void* workspace, size_t workspace_bytes, ct_stream_t stream,
                               const ct_loss_terms* terms);
int ct_multibox_loss_bwd_terms(const float* loc, const float* conf, const float* obj, const float* loc_t,
                               const float* conf_t, const uint8_t* obj_t, const float* w, const float* g,
                               int batch, int num_priors, int num_classes, float* dloc, float* dconf, float* dobj,
                               ct_stream_t stream, const ct_loss_terms* terms);

/* train.py `optimizer.step()` over the parameter groups of utils/solver.py:6-33 (torch.optim.SGD, one group per
 * tensor, maximize=False): weight decay, momentum, dampening, Nesterov and the update fused into one pass over
 * (param, grad, momentum_buf) for ALL tensors of a call (csrc/ct_optim.hip).  lr and weight_decay are per tensor (the
 * per-name multipliers of build_optimizer and the per-iteration schedule cost nothing extra); grad_scale multiplies
 * every gradient first (1 / world size in data-parallel training).
 * Arithmetic, every operation rounded separately to fp32 (no FMA), (1 - dampening) computed once on the host in fp32:
 *     g    = grad * grad_scale
 *     d    = (weight_decay != 0) ? g + weight_decay * p : g
 *     buf  = first_step ? d : momentum * buf + (1 - dampening) * d        (only when momentum != 0)
 *     step = (momentum == 0) ? d : (nesterov ? d + momentum * buf : buf)
 *     p    = p - lr * step
 * A NumPy float32 restatement of these lines reproduces the result bit for bit.
 * Transport and launch count: `items_host` is caller memory and is not read after the call returns -- the tensor
 * table travels in the kernel arguments, ct_sgd_tensors_per_launch() (80) tensors per launch, with no limit on the
 * chunks (workgroups) of a launch: a call is ceil(tensors with numel > 0 / 80) launches whatever their sizes, and none
 * when every tensor is empty.  No allocation, no host synchronisation, asynchronous on `stream`.
 * Pointers need only 4-byte alignment: a tensor whose pointers share their offset within a 16-byte line is moved in
 * 16-byte accesses with a scalar first / last group, any other tensor one dword per lane; no byte outside
 * [ptr, ptr + numel) is touched, and stores are plain vector stores.
 * n == 0 and numel == 0 are no-ops (the pointers of an empty tensor are not looked at).  CT_ERR_INVALID (nothing
 * launched): n < 0; numel < 0 or > 2^31-1; for a non-empty tensor a NULL param or grad, a NULL momentum_buf with
 * momentum != 0, or a pointer that is not 4-byte aligned; nesterov with momentum == 0 or dampening != 0 (torch's own
 * rule). */
typedef struct ct_sgd_tensor {
    float* param;          /* dev, updated in place                               */
    const float* grad;     /* dev, read only, must not alias param / momentum_buf */
    float* momentum_buf;   /* dev, NULL iff momentum == 0                         */
    int64_t numel;         /* 0 .. 2^31-1                                         */
    float lr, weight_decay;
    int first_step;        /* 1: buf := d (torch's first step), 0: recurrence     */
} ct_sgd_tensor;
int ct_sgd_tensors_per_launch(void);
int ct_sgd_step(const ct_sgd_tensor* items_host, int n, float momentum, float dampening,
                int nesterov, float grad_scale, ct_stream_t stream);

/* Gradient-norm clipping and the non-finite guard in front of ct_sgd_step: torch.nn.utils.clip_grad_norm_ (norm type 2,
 * over ALL tensors of the call) without a pass that writes the gradients and without a host synchronisation -- the
 * coefficient stays on the device, in a 16-byte ct_clip_state that ct_sgd_step_clipped reads.  Off unless called.
 * ct_grad_norm_clip arithmetic:
 *     S      = sum over every element of every tensor of (double)g * (double)g    (each product exact in binary64;
 *              summed in binary64 in an order fixed by the table: the same table gives the same bits, run after run)
 *     norm   = (float)( sqrt(S) * (double)|grad_scale| )                          one rounding to fp32
 *     finite = isfinite(norm)
 *     coef   = finite ? min(1.0f, max_norm / (norm + 1e-6f)) : 0.0f               fp32, each operation rounded once
 *     state  = { norm, coef, finite, nonfinite + !finite }
 * `nonfinite` counts the calls on this state that found a non-finite norm (the caller zeroes the state once).  A norm
 * that overflows fp32 counts as non-finite, whatever the gradients hold.  max_norm = +inf is "guard only": coef is 1
 * whenever the norm is finite.  n == 0 (or only empty tensors) gives norm 0.
 * Reduction, two levels, deterministic (no floating-point atomics, no last-arriving-workgroup finish): every workgroup
 * owns one 8192-element chunk of one tensor, found as in ct_sgd_step from a table of (grad, numel) that travels in the
 * kernel arguments, ct_grad_norm_tensors_per_launch() (220) tensors per launch; it reads the chunk in 16-byte loads
 * counted from the 16-byte line that holds element 0 (the first and the last group of a tensor element by element: no
 * byte outside [grad, grad + numel) is read), sums the squares in double, lanes and waves in a fixed order, and stores
 * one double to its own slot of `workspace`; a finishing launch of one workgroup sums the slots in a fixed order and
 * writes `state_dev` with plain vector stores.  Every slot the finish reads is written by the same call: the workspace
 * needs no clearing.  A call is ceil(tensors with numel > 0 / 220) + 1 launches; no allocation, no host
 * synchronisation, asynchronous on `stream`; `items_host` is not read after the call returns.  Gradients are never
 * written.  ct_grad_norm_workspace_bytes(items, n) is 8 bytes per chunk (at least 8; 0 for a table the call refuses).
 * CT_ERR_INVALID (nothing launched): n < 0; numel < 0 or > 2^31-1; a non-empty tensor with a NULL grad or one that is
 * not 4-byte aligned; max_norm <= 0 or NaN; a NULL state_dev; a NULL, misaligned (8 bytes) or too-small workspace.
 *
 * ct_sgd_step_clipped is ct_sgd_step with two differences:
 *   state->finite == 0: the launch updates nothing, except that it stores +0 to the momentum buffer of every tensor
 *       passed with first_step = 1, so that the buffer is defined state for the host.  A first step that was skipped
 *       therefore continues with buf = momentum * 0 + (1 - dampening) * d, which differs from torch's buf = d only
 *       when dampening != 0.
 *   otherwise gs = grad_scale * state->coef is computed once (one fp32 rounding) and the unchanged recurrence runs
 *       with gs in place of grad_scale; with coef == 1 the bits are those of ct_sgd_step.
 * Same launch count and argument errors as ct_sgd_step, plus CT_ERR_INVALID for a NULL state_dev. */
typedef struct ct_grad_tensor {
    const float* grad;     /* dev, read only */
    int64_t numel;         /* 0 .. 2^31-1    */
} ct_grad_tensor;
typedef struct ct_clip_state {
    float norm;            /* |grad_scale| * 2-norm of all gradients of the last ct_grad_norm_clip  */
    float coef;            /* what ct_sgd_step_clipped multiplies into grad_scale; 0 when !finite   */
    int finite;            /* 1: the step runs, 0: it is skipped                                    */
    int nonfinite;         /* calls on this state that found a non-finite norm                      */
} ct_clip_state;
int ct_grad_norm_tensors_per_launch(void);
size_t ct_grad_norm_workspace_bytes(const ct_grad_tensor* items_host, int n);
int ct_grad_norm_clip(const ct_grad_tensor* items_host, int n, float grad_scale, float max_norm,
                      void* workspace, size_t workspace_bytes, ct_clip_state* state_dev, ct_stream_t stream);
int ct_sgd_step_clipped(const ct_sgd_tensor* items_host, int n, float momentum, float dampening, int nesterov,
                        float grad_scale, const ct_clip_state* state_dev, ct_stream_t stream);

/* Exponential moving average of the weights ("model averaging") riding on the fused step (csrc/ct_optim.hip: the
 * step; csrc/ct_ema.hip: the rest).  Off unless called.  The update count, the decay of the step and the decision
 * whether the step is averaged at all live in a 16-byte ct_ema_state on the device, next to ct_clip_state: nothing is
 * synchronised to the host.
 * ct_ema_begin opens one update; one launch of one thread, plain loads and stores of the 16 bytes, no atomics:
 *     n       = state->updates
 *     applied = clip ? clip->finite : 1
 *     if applied:
 *         nf  = (float)n
 *         a   = 1.0f + nf
 *         b   = warmup + nf
 *         q   = a / b
 *         d   = (warmup == 0) ? decay : min(decay, q)
 *         om  = 1.0f - d
 *         state = { n == INT_MAX ? n : n + 1, d, om, 1 }
 *     else:
 *         state->applied = 0                                    nothing else is written
 * every line one fp32 rounding.  With warmup = 10 the first updates use d = 1/10, 2/11, 3/12, ... until that passes
 * `decay`; a step the non-finite guard skipped does not advance n.  The caller zeroes the state once.
 * CT_ERR_INVALID (nothing launched): a NULL or misaligned (4 bytes) state; decay outside [0, 1) or NaN; warmup other
 * than 0 or a finite value >= 1; a misaligned clip state.
 *
 * ct_sgd_step_ema is ct_sgd_step (clip NULL) or ct_sgd_step_clipped (clip given) -- the same recurrence, the same bits
 * in param and momentum_buf, the same skipped step -- and then, iff the step ran and ema_dev->applied != 0, on the new
 * parameter value still in its register:
 *     t   = d * ema
 *     u   = om * p
 *     ema = t + u
 * with d = ema_dev->decay and om = ema_dev->one_minus, three fp32 roundings, no FMA.  A skipped step, or applied == 0,
 * writes nothing to ema.  The dwordx4 path needs all four pointers (three without momentum) at one offset inside the
 * 16-byte line; any other tensor moves one dword per lane.  The table travels in the kernel arguments,
 * ct_sgd_ema_tensors_per_launch() (77) tensors per launch, no limit on n: ceil(tensors with numel > 0 / 77) launches.
 * Argument errors as ct_sgd_step, plus a NULL ema of a non-empty tensor and a NULL or misaligned ema_dev.
 *
 * ct_ema_update runs the same three lines with src in place of p, for tensors the optimizer did not touch: parameters
 * without a gradient this step, floating-point buffers such as the BatchNorm running statistics, or every tensor when
 * the optimizer is torch's.  It writes nothing when applied == 0.  ema and src must not alias.
 * ct_tensor_swap exchanges a and b element by element, to evaluate with the averaged weights in place and to put the
 * live ones back; a == b or overlapping ranges are refused on the host.
 * All three read and write no byte outside [ptr, ptr + numel), take numel == 0 with any pointers, validate the whole
 * table before any device work, allocate nothing and never synchronise; items_host is not read after the call
 * returns.  ct_ema_update and ct_tensor_swap carry 140 tensors per launch. */
typedef struct ct_ema_state {
    int updates;           /* updates applied so far (saturates at INT_MAX)                                */
    float decay;           /* d of the last applied update                                                 */
    float one_minus;       /* 1.0f - d, rounded once                                                       */
    int applied;           /* 1: the last ct_ema_begin opened an update, 0: it was a skipped step           */
} ct_ema_state;
typedef struct ct_sgd_ema_tensor {
    float* param;          /* as ct_sgd_tensor, field for field                   */
    const float* grad;
    float* momentum_buf;
    int64_t numel;
    float lr, weight_decay;
    int first_step;
    float* ema;            /* dev, updated in place; must not alias the others    */
} ct_sgd_ema_tensor;
typedef struct ct_ema_tensor {
    float* ema;            /* dev, updated in place */
    const float* src;      /* dev, read only        */
    int64_t numel;         /* 0 .. 2^31-1           */
} ct_ema_tensor;
typedef struct ct_swap_tensor {
    float* a;
    float* b;
    int64_t numel;         /* 0 .. 2^31-1           */
} ct_swap_tensor;
int ct_ema_begin(ct_ema_state* state_dev, float decay, float warmup, const ct_clip_state* clip_dev_or_null,
                 ct_stream_t stream);
int ct_sgd_ema_tensors_per_launch(void);
int ct_sgd_step_ema(const ct_sgd_ema_tensor* items_host, int n, float momentum, float dampening, int nesterov,
                    float grad_scale, const ct_clip_state* clip_dev_or_null, const ct_ema_state* ema_dev,
                    ct_stream_t stream);
int ct_ema_update(const ct_ema_tensor* items_host, int n, const ct_ema_state* ema_dev, ct_stream_t stream);
int ct_tensor_swap(const ct_swap_tensor* items_host, int n, ct_stream_t stream);

/* AdamW (decoupled weight decay; torch.optim.AdamW with amsgrad=False, maximize=False) as a second update rule on the
 * multi-tensor walk of ct_sgd_step (csrc/ct_adamw.hip).  Off unless called.  Two entries per optimizer step:
 * ct_adamw_begin advances the per-tensor step records on the device, ct_adamw_step moves the seven arrays.
 *
 * ct_adam_state is one 32-byte device record per tensor, zeroed once by the caller.  ct_adamw_begin runs one thread per
 * listed record (index_host[i] is the record's position in states_dev; the indices travel in the kernel arguments,
 * ct_adamw_begin_indices_per_launch() (1000) per launch, ceil(n / 1000) launches), plain loads and stores, no atomics.
 * With ok = clip ? clip->finite : 1:
 *     if ok:  b1p = (step == 0 ? 1.0 : beta1_pow) * beta1            binary64, one rounding
 *             b2p = (step == 0 ? 1.0 : beta2_pow) * beta2
 *             bc1 = (float)(1.0 - b1p);  bc2 = (float)(1.0 - b2p);  rs2 = sqrtf(bc2)     each rounded once
 *             record = { b1p, b2p, step == INT_MAX ? step : step + 1, 1, bc1, rs2 }
 *     else:   record.applied = 0                                      nothing else is written
 * The powers are running binary64 products: NumPy reproduces them bit for bit, and against beta ** step they are off
 * by about step * 1e-16, far below fp32 (an fp32 product would put about 1e-5 of relative error into 1 - 0.999^1).
 * ct_adamw_step takes its betas as float; a caller that wants the bias corrections to belong to exactly those values
 * passes (double)(float)beta here (ctdet.optim.FusedAdamW does): 1 - 0.999 and 1 - (float)0.999 differ by 1.3e-5.
 * CT_ERR_INVALID (nothing launched): n < 0; a NULL or misaligned (8 bytes) states_dev or a NULL index_host with n > 0;
 * a negative or repeated index; beta1 or beta2 outside [0, 1) or NaN; a misaligned clip state.
 *
 * ct_adamw_step.  Once per call on the host: om1 = (float)(1.0 - (double)beta1), om2 = (float)(1.0 - (double)beta2).
 * Per tensor: lw = lr * weight_decay (host, one fp32 rounding), a = lr / state->bc1 (device, one correctly rounded fp32
 * division, the same value in every workgroup of the tensor).  With a clip state gs = grad_scale * clip->coef, once, as
 * in ct_sgd_step_clipped; else gs = grad_scale.  Per element, one fp32 rounding per line, no FMA, sqrt and both
 * divisions correctly rounded:
 *     g   = grad * gs
 *     p   = p - lw * p                       (only when weight_decay != 0)
 *     m   = beta1 * m + om1 * g
 *     v   = beta2 * v + (om2 * g) * g
 *     den = sqrtf(v) / rs2 + eps             rs2 = state->rs2
 *     p   = p - a * (m / den)
 *     ema = d * ema + om * p                 (only with ema_dev, iff ema_dev->applied; the line of ct_sgd_step_ema)
 * A NumPy float32 restatement of these lines reproduces the result bit for bit as long as no intermediate is subnormal.
 * exp_avg and exp_avg_sq start as zeros the caller allocates: there is no first-step flag.  A skipped step
 * (clip->finite == 0) writes nothing at all: param, exp_avg, exp_avg_sq, ema and (ct_adamw_begin) the record keep their
 * bits.  Without a clip state non-finite gradients propagate as the lines say.
 * Transport as ct_sgd_step: the table travels in the kernel arguments, ct_adamw_tensors_per_launch() (59) tensors per
 * launch, ceil(tensors with numel > 0 / 59) launches; 16-byte accesses when all non-NULL pointers of a tensor share their
 * offset inside the 16-byte line, else one dword per lane; no byte outside [ptr, ptr + numel) is touched; plain vector
 * stores; the whole table is validated before any device work; no allocation, no host synchronisation; capturable.
 * CT_ERR_INVALID (nothing launched): the list of ct_sgd_step, plus, for a non-empty tensor, a NULL exp_avg, exp_avg_sq
 * or state, or a state that is not 8-byte aligned; eps < 0 or NaN; beta1 or beta2 outside [0, 1) or NaN; an ema pointer
 * without ema_dev, or ema_dev with a non-empty tensor whose ema is NULL; a misaligned clip or ema state. */
typedef struct ct_adam_state {
    double beta1_pow, beta2_pow;  /* beta^step as running binary64 products; not read while step == 0 */
    int    step;                  /* applied steps of this tensor, saturates at INT_MAX */
    int    applied;               /* 1: the last ct_adamw_begin advanced this record, 0: skipped step */
    float  bc1;                   /* (float)(1.0 - beta1_pow) */
    float  rs2;                   /* sqrtf((float)(1.0 - beta2_pow)) */
} ct_adam_state;
typedef struct ct_adamw_tensor {
    float* param;                 /* dev, updated in place */
    const float* grad;            /* dev, read only, must not alias the others */
    float* exp_avg;               /* dev, updated in place; zeros before the first step */
    float* exp_avg_sq;            /* dev, updated in place; zeros before the first step */
    float* ema;                   /* NULL unless ema_dev is given; then non-NULL for every non-empty tensor */
    const ct_adam_state* state;   /* the record ct_adamw_begin has just advanced */
    int64_t numel;                /* 0 .. 2^31-1 */
    float lr, weight_decay;
} ct_adamw_tensor;
int ct_adamw_begin_indices_per_launch(void);
int ct_adamw_begin(ct_adam_state* states_dev, const int* index_host, int n, double beta1, double beta2,
                   const ct_clip_state* clip_dev_or_null, ct_stream_t stream);
int ct_adamw_tensors_per_launch(void);
int ct_adamw_step(const ct_adamw_tensor* items_host, int n, float beta1, float beta2, float eps, float grad_scale,
                  const ct_clip_state* clip_dev_or_null, const ct_ema_state* ema_dev_or_null, ct_stream_t stream);

/* ---------------------------------------- batched test.py post-processing ---- */

/* test.py:136-161 for a batch: per (image, class>=1) select score > conf_thresh, order by
 * descending score (ties: lower prior index first), NMS, then the per-image top-k rule
 * (keep score >= k-th largest when more than max_per_image survive).
 *   boxes  dev [B,P,4] already scaled to pixels; scores dev [B,P,1+T]
 *   out_dets  dev [B, T, cap, 5]   kept rows [x1,y1,x2,y2,score] per (image,class), in
 *                                   descending score order, cap = out_cap rows reserved
 *   out_count dev [B, T]            rows valid in out_dets (after the top-k rule)
 *   out_index dev [B, T, cap]       prior index of each kept row (or NULL)
 * cap must be >= the largest number of boxes NMS keeps in any segment; on overflow the
 * call reports CT_ERR_WORKSPACE through *overflow (dev int, 0/1) for the host to check. */
size_t ct_postprocess_workspace_bytes(int batch, int num_priors, int num_fg);
int ct_postprocess_batched(const float* boxes, const float* scores, int batch, int num_priors,
                           int num_fg, float conf_thresh, float nms_thresh, int ge,
                           int max_per_image, int out_cap, float* out_dets, int* out_count,
                           int* out_index, int* overflow,
                           void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* The same with soft-NMS (ct_soft_nms_batched_dev's method / sigma / Nt / score_threshold) in place of hard NMS: every
 * candidate is selected and sorted, each segment emits at most max_per_image rows (plus ties with the last one), then the
 * same top-k rule and gather.  Same outputs, same overflow rule; rows carry their decayed scores. */
size_t ct_postprocess_soft_workspace_bytes(int batch, int num_priors, int num_fg);
int ct_postprocess_batched_soft(const float* boxes, const float* scores, int batch, int num_priors,
                                int num_fg, float conf_thresh, int method, float sigma, float Nt,
                                float score_threshold, int max_per_image, int out_cap, float* out_dets,
                                int* out_count, int* out_index, int* overflow,
                                void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* The same with Matrix NMS (ct_matrix_nms_batched_dev's method / sigma / score_threshold / pre_top) in place of hard NMS:
 * every candidate is selected and sorted, the first pre_top of each segment are decayed, each segment emits at most
 * max_per_image rows (plus ties with the last one), then the same top-k rule and gather.  Same outputs, same overflow
 * rule; rows carry their decayed scores.  conf_thresh >= 0 and score_threshold >= 0 as for the soft entry. */
size_t ct_postprocess_matrix_workspace_bytes(int batch, int num_priors, int num_fg);
int ct_postprocess_batched_matrix(const float* boxes, const float* scores, int batch, int num_priors,
                                  int num_fg, float conf_thresh, int method, float sigma,
                                  float score_threshold, int pre_top, int max_per_image, int out_cap,
                                  float* out_dets, int* out_count, int* out_index, int* overflow,
                                  void* workspace, size_t workspace_bytes, ct_stream_t stream);

/* ------------------------- flip test-time augmentation and box voting ---- */

/* Out-of-place mirror of NCHW rows: out[plane][y][j] = in[plane][y][w-1-j], planes = B*C.  in != out. */
int ct_hflip_f32(const float* in, float* out, long planes, int h, int w, ct_stream_t stream);
/* Pass k of num_passes (ct_detect_fused's boxes_k dev [B,P,4] in pixels, scores_k dev [B,P,num_cls_cols]) -> rows
 * [k*P, (k+1)*P) of every image of boxes_merged dev [B,num_passes*P,4] / scores_merged dev [B,num_passes*P,num_cls_cols].
 * mirror != 0: the pass ran on the image mirrored along W, its boxes are mirrored back in fp32: x1' = W_b - x2,
 * x2' = W_b - x1, y unchanged, W_b = scale4[0] (scale_per_image: scale4[b*4]), the image's width.  Scores are copied.
 * Post-processing the merged buffers as one image with num_passes*P priors pools the passes before NMS; its out_index
 * then holds merged indices k*P + p.  Box pointers must be 16-byte aligned. */
int ct_tta_merge(const float* boxes_k, const float* scores_k, int batch, int num_priors, int num_cls_cols,
                 int num_passes, int k, int mirror, const float* scale4, int scale_per_image,
                 float* boxes_merged, float* scores_merged, ct_stream_t stream);
/* Box voting (Detectron's box_voting, scoring method ID) on the post-processing's output, in place: the box of row r <
 * out_count[b,c] of out_dets dev [B,T,out_cap,5] becomes, per coordinate, sum(w_q x_q) / sum(w_q) over the members q of
 * (b, c): every row q < num_rows of the image with w_q = scores[b,q,1+c] > conf_thresh and IoU(row r, boxes[b,q]) >=
 * vote_thresh.  The IoU is the +1 pixel expression of the NMS (w = max(min(x2) - max(x1) + 1, 0), ovr = inter /
 * (Sa + Sb - inter)) in fp32 with the IEEE quotient; products and sums are float64, one float64 division, one rounding to
 * fp32.  A row's own source candidate is a member (IoU 1); a row without a member keeps its bits.  Scores, out_count,
 * out_index and the row order are untouched, nothing behind out_count rows is written.  boxes dev [B,num_rows,4]
 * (16-byte aligned), scores dev [B,num_rows,1+T]: the buffers the post-processing read.  0 < vote_thresh <= 1.
 * Against ct_cpu_box_vote (sequential sums): |dev - host| <= 2^-23 |host| + 2^-30 max|coordinate of the segment|; two
 * runs give the same bits.  Candidates are staged in LDS in chunks of ct_box_vote_lds_rows(); the workspace holds the
 * running sums of longer segments (not needed, and may be NULL, when num_rows <= ct_box_vote_lds_rows()). */
int ct_box_vote_lds_rows(void);
size_t ct_box_vote_workspace_bytes(int batch, int num_rows, int num_fg, int out_cap);
int ct_box_vote_batched(const float* boxes, const float* scores, int batch, int num_rows, int num_fg,
                        float conf_thresh, float vote_thresh, int out_cap, float* out_dets, const int* out_count,
                        void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* Host twin on one (image, class) segment: cand_boxes host [n,4] and weights host [n] in merged-index order, rows host
 * [m,5] updated in place (column 4 untouched).  Same fp32 IoU expression, float64 sums in candidate order. */
int ct_cpu_box_vote(const float* cand_boxes, const float* weights, int n, float vote_thresh, float* rows, int m);

/* ------------------------------------------------- PASCAL VOC evaluation ---- */

/* data/voc0712.py:339-426 (`_do_python_eval`) + data/voc_eval.py:134-203 (`voc_eval`) on the device, fed from the
 * buffers the post-processing leaves: the match rule per pipeline batch (ct_voc_match), then -- after the caller has
 * sorted the 64-bit keys -- the precision / recall curve and the AP per class (ct_voc_pr).  Host twin:
 * ctdet/evaluate.py voc_eval_lines with stable=True; the two agree bit for bit in rec, prec and the 11-point AP.
 *
 * ct_voc_match: one launch per batch, no allocation, no host synchronisation, plain vector stores.
 *   out_dets dev [B,T,cap,5], out_count dev [B,T]     as the post-processing writes them (each segment in descending
 *                                                     score order); counts are clamped to 0 .. cap
 *   image_index dev [B]                               data set index of each image; < 0 = padding image, ignored
 *   gt_boxes dev [G,4] fp32 (VOC pixel coordinates: integers, exact), gt_label dev int [G] in 1 .. T,
 *   gt_difficult dev uint8 [G], gt_off dev int [num_images+1] indexed by data set index; an image's boxes of one class
 *   keep the order of the annotation (the first maximal IoU wins, as np.argmax).  max_gt_per_image = the largest
 *   gt_off[i+1] - gt_off[i], computed by the caller: above CT_VOC_MAX_GT_PER_IMAGE the call is CT_ERR_INVALID.
 * Every kept row is first rounded the way the results files round it (data/voc0712.py:360-376):
 *   coordinate c -> rint((double)(c + 1.0f) * 10) / 10.0   == float('{:.1f}'.format(c + 1)), the + 1 in fp32 like numpy
 *   score s      -> n = rint((double)s * 1000)             == the integer '{:.3f}'.format(s) prints, half-even
 * then matched within its (image, class) segment in evaluation order -- n descending, then row ascending: the stored
 * order of a descending segment -- (voc_eval.py:160-190): IoU in double with the + 1 pixel
 * convention and the host's operation order, best = first maximum; IoU > ovthresh: a difficult box makes the row
 * neither, a free box a true positive (the box is taken), a taken box a false positive; anything else, no ground truth
 * of the class included, is a false positive.
 * Records: row number e of the image in (class, row) order goes to slot image_index * per_image_cap + e of
 *   rec_key dev int64 [num_images * per_image_cap]:  class-1 << 53 | (2^20-1 - n) << 33 | image_index << 12 | row
 *   rec_flag dev uint8 [num_images * per_image_cap]: CT_VOC_TP / CT_VOC_FP / CT_VOC_NEITHER
 * so that ascending keys = (class ascending, n descending, image ascending, row ascending) = the order a stable
 * argsort(-score) of the results lines gives.  Keys are unique; the caller fills unused slots with
 * CT_VOC_KEY_UNUSED, which sorts last.  Hence num_fg <= 1023, cap <= 4096, num_images <= 2^21.
 * status dev int [2], zeroed by the caller once: status[0] collects CT_VOC_OVERFLOW (an image has more rows than
 * per_image_cap: none of its rows is written), CT_VOC_BAD_INDEX (image_index >= num_images, or a gt_off entry outside
 * 0 .. num_gt, descending, or more than CT_VOC_MAX_GT_PER_IMAGE apart: the image is skipped) and CT_VOC_BAD_SCORE (a
 * score whose n is outside 0 .. 2^20-1 or NaN: clamped); status[1] = the largest row count of an image seen so far, the
 * per_image_cap to ask for.  Feeding one image twice is not detected: the later records replace the earlier ones. */
#define CT_VOC_MAX_GT_PER_IMAGE 1024
#define CT_VOC_MAX_THRESHOLDS 16
#define CT_VOC_KEY_UNUSED INT64_MAX
enum { CT_VOC_NEITHER = 0, CT_VOC_TP = 1, CT_VOC_FP = 2 };
enum { CT_VOC_OVERFLOW = 1, CT_VOC_BAD_INDEX = 2, CT_VOC_BAD_SCORE = 4 };
int ct_voc_match(const float* out_dets, const int* out_count, int batch, int num_fg, int cap,
                 const int* image_index, int num_images, const float* gt_boxes, const int* gt_label,
                 const uint8_t* gt_difficult, const int* gt_off, int num_gt, int max_gt_per_image,
                 double ovthresh, long long* rec_key, uint8_t* rec_flag, int per_image_cap, int* status,
                 ct_stream_t stream);
/* data/voc_eval.py:192-201 + voc_ap (:33-66): one workgroup per class c = 0 .. num_fg-1 over the rows
 * cls_off[c] .. cls_off[c+1]-1 of the sorted order.
 *   rec_flag dev uint8 [num_records]; order dev int64 [num_records] = the permutation of the key sort (row i of the
 *   sorted order has flag rec_flag[order[i]]), or NULL when rec_flag is already in sorted order
 *   cls_off dev int64 [num_fg+1] (the first sorted position of each class's keys; ascending, within 0 .. num_records)
 *   num_pos dev int [num_fg]: the class's non-difficult ground-truth boxes
 * tp / fp are scanned as integers; rec = tp / num_pos and prec = tp / max(tp + fp, DBL_EPSILON) in double go to
 * rec_out / prec_out (dev double [num_records], sorted positions; either may be NULL).  ap_out dev double [num_fg]:
 *   num_thresholds > 0: the VOC07 rule over thresholds_host (host double [num_thresholds], np.arange(0., 1.1, 0.1) for
 *     the reference's 11 points; copied into the launch): p = max prec over rec >= t, else 0; ap = ap + p / num_thresholds
 *     in threshold order -- equal to the host's value;
 *   num_thresholds == 0: the area under the monotone precision envelope; its terms equal the host's, the order of the
 *     sum differs from np.sum's pairwise order (at most (number of recall steps) * 2^-52 apart).
 * A class without rows gives 0.0; num_pos == 0 with rows gives 0.0 (11-point) / NaN (area), as on the host.
 * status dev int [1]: collects CT_VOC_BAD_INDEX for a cls_off or order entry out of range (never dereferenced). */
int ct_voc_pr(const uint8_t* rec_flag, const long long* order, long long num_records,
              const long long* cls_off, const int* num_pos, int num_fg, const double* thresholds_host,
              int num_thresholds, double* rec_out, double* prec_out, double* ap_out, int* status,
              ct_stream_t stream);

/* ------------------------------------------------------- COCO bbox evaluation ---- */

/* utils/pycocotools/cocoeval.py COCOeval(..., 'bbox') evaluate() + accumulate() (useCats = 1) and maskApi.c bbIou on the
 * device, fed from the buffers the post-processing leaves: the match rule per pipeline batch (ct_coco_match), then --
 * after the caller has sorted the 64-bit keys -- precision / recall / scores in the reference's layout
 * (ct_coco_accumulate).  Host twin: ctdet/evaluate.py coco_eval_arrays; the two agree bit for bit.
 *
 * ct_coco_match: one launch per batch, no allocation, no host synchronisation, plain vector stores.
 *   out_dets dev [B,T,cap,5], out_count dev [B,T]   as the post-processing writes them; counts are clamped to 0 .. cap.
 *                                                   A segment need not be sorted: the stable descending-score rank of
 *                                                   a row is found by counting (greater score, or equal score and a
 *                                                   smaller row number); ranks >= CT_COCO_MAX_DETS are dropped
 *   image_index dev [B]                             data set position of each image; < 0 = padding image, whose rows
 *                                                   are never read
 *   image_rank dev int [num_images] or NULL         data set position -> rank of the image by ascending image id
 *                                                   (the order COCOeval accumulates in); NULL = the identity
 *   gt_boxes dev double [G,4] as [x, y, w, h], gt_area dev double [G] (the annotation's own area), gt_iscrowd dev
 *   uint8 [G], gt_label dev int [G] in 1 .. T, gt_off dev int [num_images+1] indexed by image RANK; the boxes of one
 *   category in one image keep annotation order and are at most CT_COCO_MAX_GT_PER_SEGMENT
 *   cat_rank dev int [T]                            class c (0-based) -> position of its category on the K axis
 *   iou_thrs dev double [num_iou_thrs <= 16]        already clamped by the host: min(t, 1 - 1e-10)
 *   area_rng dev double [num_area_rng <= 4, 2]      inclusive [lo, hi]; num_iou_thrs * num_area_rng <= 64
 * A kept row [x1,y1,x2,y2,s] becomes [x1, y1, x2-x1+1, y2-y1+1] in double (data/coco.py:242-258), its area w*h.  IoU as
 * bbIou: w = min(D2+D0, G2+G0) - max(D0, G0), w <= 0 -> 0, h likewise, i = w*h, u = da for a crowd box, else
 * (da+ga)-i.  Per (threshold, area range) pair the walk of evaluateImg (cocoeval.py:256-299) in rank order: boxes
 * stably reordered with ignored ones (crowd, or annotation area outside the range) last; a matched non-crowd box is
 * skipped; the walk breaks on an ignored box once it holds a regular match; IoU < running threshold continues (an
 * equal IoU matches); the last best box wins.  An unmatched row whose area is outside the range is ignored.
 * Records: kept row of rank d in class c of the image goes to slot image_rank * per_image_cap + e, e = (kept rows of
 * the image's classes before c) + d:
 *   rec_key dev int64:  cat_rank << 56 | ~(order-preserving 32-bit image of the float32 score) << 24 | image_rank << 7 | d
 *   rec_matched / rec_ignored dev uint64: bit (t * num_area_rng + a) = the row is matched / ignored for that pair
 * Ascending keys = (category, score descending, image rank, rank in segment) = the stable argsort(-score) of
 * accumulate() over the images in ascending id.  Keys are unique and 63 bits wide; the caller fills unused slots with
 * CT_COCO_KEY_UNUSED, which sorts last.  Hence T and K <= 127, num_images <= 131072, cap <= 4096.
 * status dev int [2], zeroed by the caller once: status[0] collects CT_COCO_OVERFLOW (an image keeps more rows than
 * per_image_cap: none of them is written), CT_COCO_BAD_INDEX (image_index >= num_images, an image_rank, gt_off or
 * cat_rank entry out of range, or more than CT_COCO_MAX_GT_PER_SEGMENT boxes in a segment: skipped) and
 * CT_COCO_BAD_SCORE (a NaN score); status[1] = the largest number of kept rows of an image so far, the per_image_cap to
 * ask for.  Feeding one image twice is not detected: the later records replace the earlier ones. */
#define CT_COCO_MAX_GT_PER_SEGMENT 256
#define CT_COCO_MAX_DETS 100
#define CT_COCO_MAX_IOU_THRS 16
#define CT_COCO_MAX_AREA_RNG 4
#define CT_COCO_MAX_REC_THRS 128
#define CT_COCO_MAX_CATEGORIES 127
#define CT_COCO_MAX_IMAGES 131072
#define CT_COCO_ACC_CHUNK 512
#define CT_COCO_KEY_UNUSED INT64_MAX
enum { CT_COCO_OVERFLOW = 1, CT_COCO_BAD_INDEX = 2, CT_COCO_BAD_SCORE = 4 };
int ct_coco_match(const float* out_dets, const int* out_count, int batch, int num_fg, int cap,
                  const int* image_index, const int* image_rank, int num_images, const double* gt_boxes,
                  const double* gt_area, const uint8_t* gt_iscrowd, const int* gt_label, const int* gt_off,
                  int num_gt, const int* cat_rank, const double* iou_thrs, int num_iou_thrs,
                  const double* area_rng, int num_area_rng, long long* rec_key,
                  unsigned long long* rec_matched, unsigned long long* rec_ignored, int per_image_cap,
                  int* status, ct_stream_t stream);
/* cocoeval.py:315-418 (accumulate): one workgroup per (category k, area range a, limit m), one wave per IoU threshold,
 * over the rows cat_off[k] .. cat_off[k+1]-1 of the sorted order whose rank in their segment is < max_dets[m] (one
 * sort serves every limit: a subsequence of a sorted list is sorted).
 *   rec_key / rec_matched / rec_ignored dev [num_records]; order dev int64 [num_records] = the permutation of the key
 *   sort, or NULL when the records are already in sorted order
 *   cat_off dev int64 [K+1] (first sorted position of each category's keys; ascending, within 0 .. num_records)
 *   npig dev int [K, num_area_rng]: the category's non-crowd boxes with lo <= area <= hi
 *   max_dets dev int [num_max_dets <= 4]; rec_thrs dev double [num_rec_thrs <= 128], ascending
 * tp / fp are scanned as integers in chunks of CT_COCO_ACC_CHUNK rows with a carry; rc = tp / npig and
 * pr = tp / ((fp + tp) + DBL_EPSILON) in double, the maximum of pr from the right, then for every recall threshold the
 * envelope and the score at the first row with rc >= threshold, 0 where there is none.  Written in the reference's
 * layout: precision, scores dev double [T,R,K,A,M], recall dev double [T,K,A,M] (the last rc, 0 without rows); -1
 * everywhere for a (k, a) with npig == 0.
 * status dev int [1]: collects CT_COCO_BAD_INDEX for a cat_off or order entry out of range (never dereferenced). */
int ct_coco_accumulate(const long long* rec_key, const unsigned long long* rec_matched,
                       const unsigned long long* rec_ignored, const long long* order, long long num_records,
                       const long long* cat_off, const int* npig, int num_categories, int num_area_rng,
                       const int* max_dets, int num_max_dets, int num_iou_thrs, const double* rec_thrs,
                       int num_rec_thrs, double* precision, double* recall, double* scores, int* status,
                       ct_stream_t stream);

/* ------------------------------------------------------------ convolution ---- */

/* One fused convolution of the RFBNet-VGG stack.  Replaces the ATen sequence
 * Conv2d [+ bias] [-> BatchNorm2d(eval)] [-> *res_scale + residual] [-> ReLU] [-> cat / permute]
 * of models/RFB_Net_vgg.py:7-22 (BasicConv), :53-64 / :100-112 (RFB tail), :219-227 (VGG),
 * :238-248 (heads: permute(0,2,3,1) + flatten + cat), as one implicit-GEMM kernel on the
 * fp32 MFMA path (v_mfma_f32_32x32x2_f32; exact fp32 products, fp32 accumulate).
 *
 * y[n,co,oh,ow] = act( (sum_k w[co,k] x[n,k@(oh,ow)]) * scale[co] + shift[co] ) with the
 * optional residual  y = act( (.)*res_scale + res[n,co,oh,ow] ).
 */
typedef struct ct_out_segment {
    float* ptr;          /* dev */
    int co_begin;        /* output channels [co_begin, co_end) go to this segment */
    int co_end;
    int pix_stride;      /* floats between consecutive pixels (= #channels of the segment) */
    long long img_stride;/* floats between consecutive images */
    long long base;      /* float offset of pixel 0 / channel co_begin inside an image */
} ct_out_segment;

typedef struct ct_conv_desc {
    /* input: NCHW buffer with in_ctot channels; the conv reads channels [in_coff, in_coff+cin) */
    const float* in;
    int batch, cin, h, w, in_ctot, in_coff;
    /* packed weights from ct_conv_pack_weights(): [k_pad][m_pad]; scale/shift: [m_pad] */
    const float* wpacked;
    const float* scale;
    const float* shift;
    int cout, m_pad, k_pad;
    int kh, kw, stride, pad_h, pad_w, dil;
    int oh, ow;
    /* output mode 0: NCHW buffer with out_ctot channels, written at [out_coff, out_coff+cout) */
    float* out;
    int out_ctot, out_coff;
    /* optional residual (NCHW, res_ctot channels, offset res_coff); NULL = none */
    const float* res;
    int res_ctot, res_coff;
    float res_scale;
    int relu;            /* 1: ReLU on every output channel */
    const float* lo;     /* optional dev [m_pad]: y = max(y, lo[co]) per channel (0 = ReLU, -inf = none);
                            overrides `relu`; lets convs with and without ReLU share one launch */
    /* output mode 1 (nseg > 0): channels-last scatter into up to 3 flattened head buffers */
    int nseg;
    ct_out_segment seg[3];
    /* tile configuration: 0 = heuristic; otherwise 1 + index into ct_conv_num_configs() */
    int config;
    /* 1: data gradient of the convolution (conv_transpose): `in` = dY [batch,cin=cout_fwd,h,w],
     * output = dX [batch,cout=cin_fwd,oh,ow] with (oh,ow) the forward INPUT size, weights packed by
     * ct_conv_pack_weights_dgrad; stride/pad/dil are the forward convolution's.  What autograd's
     * conv backward-data does for every Conv2d of models/RFB_Net_vgg.py in train.py:228. */
    int transposed;
    /* split-K for maps too small to fill the chip (ct_conv2d_fwd only): ksplit > 1 divides the reduction
     * (cin * kh * kw) over that many workgroups per output tile; each writes its partial sums to its own slab
     * of ksplit_ws ([ksplit][cout][batch*oh*ow] floats, no atomics) and a finishing kernel adds the slabs in
     * order and applies the epilogue, so results do not depend on scheduling.  ksplit_ws_floats = capacity of
     * the workspace (the factor is clamped to what fits).  0 / 1 or a null workspace = off; -1 = let the
     * library choose from the number of output tiles. */
    int ksplit;
    float* ksplit_ws;
    long long ksplit_ws_floats;
    /* Maxima of |activation| for the f16x2 operand form (csrc/ct_f16x2.h: binary16 pieces need a power-of-two scale, taken from
     * the tensor's maximum).  Both optional (NULL = off), both arrays of `batch` LINES of CT_ABSMAX_LINE_BYTES bytes of device
     * memory that the caller zeroes once per step: the bit pattern of max |x| of image n lives in the first word of line n.  PER
     * IMAGE, so that what a kernel computes for an image never depends on the other images of its batch.
     *   in_absmax   per image an upper bound of |x| over the input slice, left there by whoever produced the input (any kernel of
     *               this library run with out_absmax, or ct_absmax_f32); kernels that need the maxima and do not get them take
     *               them themselves in an extra pass (ct_conv2d_wino4s_fwd variant 3) or refuse (ct_conv2d_wino4f_pool_fwd_v
     *               variant 2, the "h2:" configurations of ct_conv2d_x3_fwd);
     *   out_absmax  the launch folds max |y| of everything it stores for image n into line n (atomic max): honoured by the shared
     *               epilogue of ct_conv2d_wino4s_fwd (every variant) and of the f16x2 variant of ct_conv2d_wino4f_pool_fwd_v, by
     *               ct_conv2d_x3_fwd and ct_conv2d_fwd (every configuration; split-K launches: in the finishing kernel); ignored
     *               by the other kernels (the fp32 / bf16x3 fused Winograd kernels, the bf16 path) and by data-gradient launches.
     * Range of the f16x2 kernels: any VALID bound in in_absmax (>= the true maximum; results within the library's 1e-4 for bounds
     * up to 2^10 x the maximum) and any normal fp32 magnitude of activations and weights for which the fp32 / bf16x3 kernels
     * themselves stay finite: the power-of-two scales follow the maxima over fp32's whole exponent range and are undone as two
     * exact factors (csrc/ct_f16x2.h, unscale_for), so conv(x 2^a, w 2^b) = conv(x, w) 2^(a + b) bit for bit wherever no value
     * leaves fp32's normal range (maxima below 2^-112: still within 1e-4, no longer bit-covariant).  What the form does NOT
     * give: the low bits of ordinary values next to an outlier in the same image -- one value 2^20 x the rest costs the
     * Winograd forms 5e-4 of the other outputs' range (2^14: 8e-6; the bf16x3 twins: 5e-7; tests/test_gpu_f16x2_range.py). */
    const unsigned* in_absmax;
    unsigned* out_absmax;
} ct_conv_desc;
#define CT_ABSMAX_LINE_BYTES 128
/* max |x| over the channel slice [per_image floats] of every image (images img_stride floats apart), folded into `lines`
 * (batch lines, atomic max; the caller zeroes them once per step). */
int ct_absmax_f32(const float* in, int batch, long long per_image, long long img_stride, unsigned* lines, ct_stream_t stream);

/* Rows of the packed weight matrix for a (cin, kh, kw) filter: k_pad. */
int ct_conv_kpad(int cin, int kh, int kw);
int ct_conv_mpad(int cout);
int ct_conv_num_configs(void);
/* Human-readable name of tile config i (0-based), e.g. "128x128".  The last one, "valu", is not an implicit-GEMM tile:
 * conv_valu3x3_f32, the 3x3 / 3-input-channel image layer (models/RFB_Net_vgg.py:219, conv1_1) on the vector ALU; it
 * is what config 0 picks for such a layer (cout % 8 == 0, NCHW output, no residual) and CT_ERR_UNSUPPORTED elsewhere. */
const char* ct_conv_config_name(int i);
/* Pack nparts (1..6) weight tensors w[i] dev [cout_i, cin, kh, kw] (concatenated along cout) into
 * wpacked dev [k_pad][m_pad] (k = ci*kh*kw + tap, zero padded). */
int ct_conv_pack_weights(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw,
                         float* wpacked, int m_pad, int k_pad, ct_stream_t stream);
/* Same for the data-gradient launch: wpacked [k_pad][m_pad] with k = co*kh*kw + tap over the
 * concatenated couts and m = ci;  k_pad = ct_conv_kpad(sum cout, kh, kw), m_pad = ct_conv_mpad(cin). */
int ct_conv_pack_weights_dgrad(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw,
                               float* wpacked, int m_pad, int k_pad, ct_stream_t stream);
/* Epilogue vectors. BatchNorm2d(eval) of models/RFB_Net_vgg.py:13: scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale.  With gamma == NULL: scale = 1, shift = bias (or 0 if bias NULL).
 * Written at [offset, offset+n) of the m_pad-long vectors. */
int ct_conv_fold_epilogue(const float* gamma, const float* beta, const float* mean, const float* var,
                          float eps, const float* bias, int n, int offset,
                          float* scale, float* shift, ct_stream_t stream);
int ct_conv2d_fwd(const ct_conv_desc* desc, ct_stream_t stream);

/* Winograd F(2x2,3x3) variant of ct_conv2d_fwd for 3x3 / stride 1 / dilation 1 / pad 1 convolutions with
 * cin % 8 == 0 and an NCHW output (the VGG trunk and the 3x3 BasicConv layers, models/RFB_Net_vgg.py:7-22,
 * 219-227): same descriptor, same fused epilogue, 2.25x fewer multiplications.  `desc->wpacked/k_pad/m_pad`
 * are ignored; the weights come pre-transformed (U = G g G^T) from ct_conv_pack_weights_wino. */
int ct_conv_wino_supported(const ct_conv_desc* desc);
size_t ct_conv_wino_packed_floats(int cin, int cout);
int ct_conv_pack_weights_wino(const float* const* w, const int* cout, int nparts, int cin, float* upacked,
                              ct_stream_t stream);
int ct_conv2d_wino_fwd(const ct_conv_desc* desc, const float* upacked, ct_stream_t stream);
/* Same with the following MaxPool2d(2, 2[, ceil_mode]) (models/RFB_Net_vgg.py:328-330) fused: the 2x2 Winograd
 * output tile is the pooling window, so the pooled activation [B, pool_ctot, pool_oh, pool_ow] (channels at
 * pool_coff) is written from registers; write_full = 0 skips the full-resolution output when nothing else reads it.
 * pool_oh/ow = floor or ceil of oh/2, ow/2 (ceil_mode windows are clipped to the map). */
int ct_conv2d_wino_pool_fwd(const ct_conv_desc* desc, const float* upacked, float* pool_out, int pool_ctot,
                            int pool_coff, int pool_oh, int pool_ow, int write_full, ct_stream_t stream);
/* Weights of the DATA-GRADIENT convolution of a 3x3 / stride 1 / pad 1 layer (input channels = sum cout,
 * output channels = cin, taps rotated by 180 degrees), for ct_conv2d_wino_fwd on dY:
 * upacked holds ct_conv_wino_packed_floats(sum cout, cin) floats. */
int ct_conv_pack_weights_wino_dgrad(const float* const* w, const int* cout, int nparts, int cin,
                                    float* upacked, ct_stream_t stream);

/* Winograd F(4x4,3x3): the large-tile variant of the five entry points above, same contracts (same layers:
 * models/RFB_Net_vgg.py:7-22,219-227; same descriptor, epilogue, pooling fusion -- a 4x4 tile holds four pooling
 * windows -- and head scatter), its own packed layout (ct_conv_wino4_packed_floats floats).  36 multiplications per
 * 16 outputs: 4x fewer than the direct convolution, 1.78x fewer than F(2x2,3x3); fp32 rounding error about 2e-6 of
 * the output range (interpolation points 0, +-3/4, +-3/2, inf: csrc/ct_wino4_points.h) against 1e-6 for F(2x2,3x3).
 * desc->ksplit / ksplit_ws are honoured by ct_conv2d_wino4_fwd as a split over INPUT CHANNELS (ksplit -1: the library
 * decides, > 1: that many slices, else off): each slice stores its output-transformed partial sums in its slab
 * ws[slice][cout][batch*oh*ow] and a finishing kernel adds them in slice order -- for maps whose 32-tile x 64-cout
 * workgroup grid cannot fill the chip (small batches).  Not combined with the fused pooling.
 * ksplit -2 (with ksplit_ws >= 256*2*64*32*16 floats): stream-K -- the caller promises the launch runs alone on the
 * device; a persistent grid of 256 workgroups does the full rounds of work items whole and cuts the last, partial round
 * by input-channel chunks (partial sums in slabs, a fix-up kernel adds them in chunk order and applies the epilogue,
 * fused pooling included).  Deterministic, but the cut items are the last tiles of the batch: an image's rounding then
 * depends on its batch position, which is why ctdet/engine.py only uses it on request (CTDET_W4_STREAMK=1). */
int ct_conv_wino4_supported(const ct_conv_desc* desc);
size_t ct_conv_wino4_packed_floats(int cin, int cout);
int ct_conv_pack_weights_wino4(const float* const* w, const int* cout, int nparts, int cin, float* upacked,
                               ct_stream_t stream);
int ct_conv_pack_weights_wino4_dgrad(const float* const* w, const int* cout, int nparts, int cin,
                                     float* upacked, ct_stream_t stream);
int ct_conv2d_wino4_fwd(const ct_conv_desc* desc, const float* upacked, ct_stream_t stream);
int ct_conv2d_wino4_pool_fwd(const ct_conv_desc* desc, const float* upacked, float* pool_out, int pool_ctot,
                             int pool_coff, int pool_oh, int pool_ow, int write_full, ct_stream_t stream);

/* Winograd F(2x2,3x3) on the bf16 matrix pipe (csrc/ct_wino_x3.hip): the entry points of ct_conv2d_wino_fwd above with
 * the transform-domain products evaluated as six bf16 piece products ("bf16x3", see below) on v_mfma_f32_32x32x16_bf16
 * -- same layers (models/RFB_Net_vgg.py:7-22,219-227,238-248), descriptor, epilogue, pooling fusion and head scatter;
 * cin % 16 == 0.  The weights come pre-transformed AND pre-split from ct_conv_pack_weights_wino_x3
 * (ct_conv_wino_x3_packed_bytes bytes).  `variant` must be 1: eight-wave workgroups, the hi.hi products accumulate in their own
 * register block (the large sum sees cin / 16 roundings; error vs fp64 about a third of ct_conv2d_wino_fwd's, a tenth of
 * ct_conv2d_wino4_fwd's).  (Variant 2 of rounds 4-5 -- four-wave workgroups, one accumulator -- was removed in round 6: it
 * never won a layer inside the two-stream pipeline; CT_ERR_INVALID.) */
int ct_conv_wino_x3_supported(const ct_conv_desc* desc);
size_t ct_conv_wino_x3_packed_bytes(int cin, int cout);
int ct_conv_pack_weights_wino_x3(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                 ct_stream_t stream);
int ct_conv_pack_weights_wino_x3_dgrad(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                       ct_stream_t stream);
int ct_conv2d_wino_x3_fwd(const ct_conv_desc* desc, const void* upacked, int variant, ct_stream_t stream);
int ct_conv2d_wino_x3_pool_fwd(const ct_conv_desc* desc, const void* upacked, int variant, float* pool_out, int pool_ctot,
                               int pool_coff, int pool_oh, int pool_ow, int write_full, ct_stream_t stream);

/* Winograd F(4x4,3x3) in three kernels with the transform-domain GEMMs on the bf16 matrix pipe (csrc/ct_wino4s.hip): the
 * wide 3x3 layers of the VGG trunk and the multibox heads (models/RFB_Net_vgg.py:219-227 conv3_x .. conv5_x, :238-248)
 * -- same descriptor, transforms (interpolation points 0, +-3/4, +-3/2, inf), epilogue, pooling fusion and head scatter as
 * ct_conv2d_wino4_fwd, fp32 results equal to it up to summation order; cin % 16 == 0.  An input-transform kernel writes
 * V = B^T d B once per (tile, channel), split exactly into three bfloat16 pieces, as MFMA operand fragments; 36 GEMMs
 * M[xi] = U[xi] V[xi] (128 x 128 blocks, operands by LDS-DMA, six piece products per multiply-add, no vector-ALU work in
 * the loop); an output-transform kernel applies A^T M A and the epilogue.  V and M live in the caller's `workspace`
 * (ct_conv_wino4s_workspace_bytes(desc) bytes: 13.5 bytes per (output pixel, input channel) + 9 per (output pixel,
 * output channel); launches on different streams need different workspaces).  Weights: ct_conv_pack_weights_wino4s
 * (ct_conv_wino4s_packed_bytes bytes).  variant 1: bf16x3, the hi.hi products in their own accumulator (variant 2 of
 * rounds 4-5, one accumulator, was removed in round 6: CT_ERR_BAD_ARG).
 * variant 3 (round 6): the "f16x2" operand form -- every transform-domain value as TWO binary16 pieces (hi = rne16(x 2^e),
 * lo = rne16(x 2^e - hi)) and a multiply-add as the THREE piece products hi.hi, hi.lo, lo.hi on the f16 matrix pipe, the hi.hi
 * products in their own accumulator: the same 22-24 bits as three bfloat16 pieces / six products (same error against fp64), half
 * the matrix instructions, 9 instead of 13.5 bytes of V per (output pixel, input channel).  The power-of-two scales 2^e come from
 * the operands' own maxima (an absmax pass over the input slice in front of the input transform; max |g| of the layer at
 * packing time), so no binary16 piece overflows for any data; the output transform undoes them exactly.  Weights for variant 3:
 * ct_conv_pack_weights_wino4s_h2 (ct_conv_wino4s_h2_packed_bytes bytes; not recordable by ct_pack_record_begin). */
int ct_conv_wino4s_supported(const ct_conv_desc* desc);
size_t ct_conv_wino4s_packed_bytes(int cin, int cout);
size_t ct_conv_wino4s_h2_packed_bytes(int cin, int cout);
/* Batched f16x2 packing for callers that re-pack many layers per step (the training engine, once per optimizer step): fill one
 * item per layer on the host (ct_conv_wino_h2_pack_item_bytes() bytes each; tile 47 = the layout of ct_conv_pack_weights_wino4s_h2,
 * 48 = of ct_conv_pack_weights_wino4f_h2; dgrad != 0 = the data-gradient layouts), copy the items to the device as one array and
 * replay it with ct_conv_wino_h2_pack_run: three launches for the whole list (trailers, maxima, packing) instead of three per
 * layer.  Same bytes as the per-layer calls. */
size_t ct_conv_wino_h2_pack_item_bytes(void);
int ct_conv_wino_h2_pack_item(const float* const* w, const int* cout, int nparts, int cin, int dgrad, int tile, void* upacked,
                              void* item_out);
int ct_conv_wino_h2_pack_run(const void* items_dev, int n, ct_stream_t stream);
size_t ct_conv_wino4s_workspace_bytes(const ct_conv_desc* desc);
int ct_conv_pack_weights_wino4s(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                ct_stream_t stream);
int ct_conv_pack_weights_wino4s_dgrad(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                      ct_stream_t stream);
int ct_conv_pack_weights_wino4s_h2(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                   ct_stream_t stream);
int ct_conv_pack_weights_wino4s_h2_dgrad(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                         ct_stream_t stream);
int ct_conv2d_wino4s_fwd(const ct_conv_desc* desc, const void* upacked, void* workspace, size_t workspace_bytes,
                         int variant, ct_stream_t stream);
int ct_conv2d_wino4s_pool_fwd(const ct_conv_desc* desc, const void* upacked, void* workspace, size_t workspace_bytes,
                              int variant, float* pool_out, int pool_ctot, int pool_coff, int pool_oh, int pool_ow,
                              int write_full, ct_stream_t stream);

/* Winograd F(4x4,3x3) FUSED with the transform-domain products on the bf16 matrix pipe (csrc/ct_wino4f.hip): the narrow
 * 3x3 layers on the large maps (models/RFB_Net_vgg.py:323-336 conv1_2 .. conv3_1; conv3_2 / conv3_3 at 512 x 512), where the
 * three-kernel form's workspace traffic does not pay and the fp32-MFMA kernel is bound by the slowest matrix rate -- same
 * descriptor, transforms, epilogue, pooling fusion and head scatter as ct_conv2d_wino4_fwd, fp32 results equal to it up to
 * summation order; cin % 16 == 0.  One workgroup = 32 tiles x one block of 64 couts: patches arrive in LDS by DMA, the
 * transform runs once per (tile, channel, 64 couts), V stays in LDS as fp32 and is split into the three bfloat16 pieces by
 * the wave that multiplies it; no workspace.  Weights: ct_conv_pack_weights_wino4f (ct_conv_wino4f_packed_bytes bytes). */
int ct_conv_wino4f_supported(const ct_conv_desc* desc);
size_t ct_conv_wino4f_packed_bytes(int cin, int cout);
int ct_conv_pack_weights_wino4f(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                ct_stream_t stream);
int ct_conv_pack_weights_wino4f_dgrad(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                      ct_stream_t stream);
int ct_conv2d_wino4f_fwd(const ct_conv_desc* desc, const void* upacked, ct_stream_t stream);
int ct_conv2d_wino4f_pool_fwd(const ct_conv_desc* desc, const void* upacked, float* pool_out, int pool_ctot, int pool_coff,
                              int pool_oh, int pool_ow, int write_full, ct_stream_t stream);
/* The same kernel on the f16x2 operand form (variant 2; variant 1 = bf16x3 = ct_conv2d_wino4f_pool_fwd): two binary16 pieces per
 * transform-domain value, three piece products (csrc/ct_f16x2.h, see ct_conv2d_wino4s_fwd variant 3) -- 27 instead of 54 MFMAs and
 * 120 instead of 220 split instructions per wave and 16-channel chunk.  Needs desc->in_absmax (the fused kernel cannot take the
 * input's maximum itself) and weights from ct_conv_pack_weights_wino4f_h2 (ct_conv_wino4f_h2_packed_bytes bytes); pool_out == NULL
 * and write_full == 1 for a plain launch.  Honours desc->out_absmax. */
size_t ct_conv_wino4f_h2_packed_bytes(int cin, int cout);
int ct_conv_pack_weights_wino4f_h2(const float* const* w, const int* cout, int nparts, int cin, void* upacked, ct_stream_t stream);
int ct_conv_pack_weights_wino4f_h2_dgrad(const float* const* w, const int* cout, int nparts, int cin, void* upacked,
                                         ct_stream_t stream);
int ct_conv2d_wino4f_pool_fwd_v(const ct_conv_desc* desc, const void* upacked, int variant, float* pool_out, int pool_ctot,
                                int pool_coff, int pool_oh, int pool_ow, int write_full, ct_stream_t stream);
/* The launches without residual, per-channel floor and head scatter run an epilogue that works out a tile's geometry once per work
 * item; CTDET_W4F_LEAN_EPI=0 (read once per process) keeps the per-row epilogue of the other launches instead -- same bits, for the
 * A/B.  This call overrides the variable inside a process: on = 1 / 0, negative = back to the environment's choice.  Not
 * synchronised with launches in flight on other threads beyond the flag itself. */
int ct_wino4f_set_lean_epilogue(int on);

/* ---- "bf16x3": the fp32 convolution of ct_conv2d_fwd on the bf16 matrix pipe (csrc/ct_conv_x3.hip) ----
 * Same layers (models/RFB_Net_vgg.py:7-22 BasicConv, the plain Conv2d layers, the multibox heads :238-248), the same
 * descriptor (NCHW fp32 in / out, channel slices, residual, per-channel floor, head scatter, ksplit slabs) and the
 * same results to fp32 accuracy: every fp32 operand is split exactly into three bfloat16 pieces and the six leading
 * piece products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (six bf16 MFMAs = 0.375 of one fp32 MFMA;
 * per-layer error against fp64 no worse than ct_conv2d_fwd's, tests/test_gpu_x3.py).  Any filter size / stride /
 * dilation; cin must be a multiple of the config's k-step (CT_ERR_UNSUPPORTED otherwise).  desc->transposed = 1 (the
 * data gradient, ct_conv2d_fwd's contract: `in` = dY, weights from ct_conv_pack_weights_x3_dgrad, stride 1 or 2) is
 * what `losses.backward()` (train.py:228) needs for the same layers.  desc->wpacked / m_pad / k_pad / config are ignored: the split weights come from
 * ct_conv_pack_weights_x3 for the k-step length (16 or 32 channels) of the chosen tile config. */
int ct_conv_x3_num_configs(void);
const char* ct_conv_x3_config_name(int i);               /* e.g. "x3:128x128k16" */
int ct_conv_x3_config_bk(int i);                         /* channels per k-step of config i */
size_t ct_conv_x3_packed_bytes(int cin, int cout, int kh, int kw, int bk);
int ct_conv_pack_weights_x3(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk,
                            void* wx3, ct_stream_t stream);
/* Data-gradient layout: rows = cin (forward input channels), k-channels = the concatenated couts; holds
 * ct_conv_x3_packed_bytes(sum cout, cin, kh, kw, bk) bytes. */
int ct_conv_pack_weights_x3_dgrad(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk,
                                  void* wx3, ct_stream_t stream);
int ct_conv2d_x3_fwd(const ct_conv_desc* desc, const void* wx3, int config, ct_stream_t stream);
/* The f16x2 operand form of the same kernel (csrc/ct_f16x2.h; see ct_conv2d_wino4s_fwd variant 3): configurations named
 * "h2:<tile>" (ct_conv_x3_config_h2(i) == 1) take weights from ct_conv_pack_weights_x3h (ct_conv_x3h_packed_bytes bytes: two
 * binary16 pieces of w 2^eW and a trailer with eW) and need desc->in_absmax; forward only.  Every configuration honours
 * desc->out_absmax (split-K launches: in their finishing kernel). */
int ct_conv_x3_config_h2(int i);
/* The pointwise form of the "h2:" configurations: forward 1x1 / stride 1 / dilation 1 / pad 0 launches with cin % 32 == 0, no
 * split-K and no head scatter (nseg == 0) run conv_x3_f32_pw -- one barrier per 32 input channels, weights by LDS-DMA, no filter
 * geometry -- whose results are bit-identical to the generic kernel's; everything else keeps the generic kernel.  Process-wide
 * switch, initial value from CTDET_X3_POINTWISE (read once; default 1).  Returns the previous value.  Set it before a graph is
 * captured, not between capture and replay. */
int ct_conv_x3_pointwise_enable(int on);
size_t ct_conv_x3h_packed_bytes(int cin, int cout, int kh, int kw, int bk);
int ct_conv_pack_weights_x3h(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk, void* wx3,
                             ct_stream_t stream);
/* All weight splits of a training step (train.py:222-229 updates every weight every step) in ONE launch: the arguments
 * never change between steps, so build the list once -- ct_conv_x3_pack_item fills one item of
 * ct_conv_x3_pack_item_bytes() bytes in HOST memory from the arguments of ct_conv_pack_weights_x3 (dgrad = 0) or
 * ct_conv_pack_weights_x3_dgrad (dgrad = 1) without launching --, copy the items to the device, and replay them with
 * ct_conv_x3_pack_run(items_dev, n). */
size_t ct_conv_x3_pack_item_bytes(void);
int ct_conv_x3_pack_item(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw, int bk, void* wx3,
                         int dgrad, void* host_item);
int ct_conv_x3_pack_run(const void* items_dev, int n, ct_stream_t stream);

/* ---- bf16 channels-last convolutions (BASELINE.json configs[4]: "bf16 MFMA convs + fp32 NMS") ----
 * Same layers and epilogue as ct_conv2d_fwd (models/RFB_Net_vgg.py:7-22,219-248), other storage: activations
 * are [batch][h][w][channels] bfloat16 (round-to-nearest-even of the fp32 value), accumulation and epilogue
 * in fp32.  The descriptor is ct_conv_desc with `in`, `out`, `res` pointing at bf16 NHWC buffers (channel
 * slices: in_ctot / in_coff / cin multiples of 8), `wpacked` from ct_conv_pack_weights_bf16, `scale` / `shift`
 * / `lo` fp32, segments (nseg > 0) written in fp32 exactly as by ct_conv2d_fwd; ksplit / ksplit_ws as for
 * ct_conv2d_fwd (slabs [ksplit][batch*oh*ow][cout] fp32); m_pad / k_pad / config / transposed unused. */
int ct_conv_bf16_cin_pad(int cin);
int ct_conv_bf16_cout_pad(int cout);
/* bf16 elements of the packed weights of a (cin, cout, kh, kw) filter bank */
size_t ct_conv_bf16_packed_elems(int cin, int cout, int kh, int kw);
int ct_conv_pack_weights_bf16(const float* const* w, const int* cout, int nparts, int cin, int kh, int kw,
                              void* wpacked, ct_stream_t stream);
int ct_conv2d_bf16_fwd(const ct_conv_desc* d, ct_stream_t stream);
/* The kernel variant ct_conv2d_bf16_fwd launches for `d` under the current CTDET_BF16_BIG_MIN / CTDET_BF16_SHORTK (read per
 * call) and CTDET_BF16_BK (read once per process): "bf16:<pixels>x<couts>k<channels per k-step>", a trailing "s" for the image
 * layer (cin_pad == 8, a k-step of four taps) -- bf16:128x64k32s, bf16:128x128k32s, bf16:256x256k32, bf16:128x64k32 (short-K),
 * bf16:128x64k64, bf16:128x128k32 (CTDET_BF16_BK=32, three-buffer ring), bf16:128x128k64.  Pure host code (no HIP call): the
 * launcher picks by the same function.  NULL, with ct_last_error_string set, for a descriptor the launcher refuses. */
const char* ct_conv_bf16_variant_name(const ct_conv_desc* d);
/* x dev [batch][channels][hw] fp32 -> y dev [batch][hw][c_pad] bf16 (channels >= `channels` zero) and back
 * (channel slice [coff, coff+channels) of a ctot-channel NHWC buffer -> dense NCHW fp32) */
int ct_nchw_f32_to_nhwc_bf16(const float* x, int batch, int channels, int hw, int c_pad, void* y, ct_stream_t stream);
int ct_nhwc_bf16_to_nchw_f32(const void* y, int batch, int channels, int hw, int ctot, int coff, float* x,
                             ct_stream_t stream);
/* nn.MaxPool2d on an NHWC bf16 map (models/RFB_Net_vgg.py:331-341); oh/ow decide floor or ceil mode */
int ct_maxpool2d_nhwc_bf16(const void* x, void* y, int batch, int channels, int h, int w, int oh, int ow, int k,
                           int stride, int pad, ct_stream_t stream);

/* Winograd F(4x4,3x3) for the bf16 channels-last path (csrc/ct_wino_bf16.hip): the wide 3x3 layers of the VGG trunk
 * (models/RFB_Net_vgg.py:219-227) with 4x fewer multiplications than ct_conv2d_bf16_fwd.  Same storage and descriptor (bf16 NHWC
 * `in` / `out` with channel slices, fp32 `scale` / `shift`, `relu`); `wpacked` comes from ct_conv_pack_weights_bf16_wino.  The
 * transform-domain operands are SINGLE binary16 values on v_mfma_f32_32x32x16_f16 (eleven significant bits: bfloat16 there costs
 * 6-8x the direct kernel's error), V scaled by one power of two per image taken from the maxima lines (ct_conv_desc.in_absmax,
 * csrc/ct_f16x2.h), U by one per layer taken from max |g| at packing time; the output transform undoes both exactly.  Three
 * launches: input transform (V = B^T d B as MFMA fragments), 36 GEMMs M = V U with fp32 accumulation, output transform + epilogue
 * (rounded once to bf16).  V, M and -- when in_absmax is NULL -- the maxima lines live in the caller's workspace
 * (ct_conv_bf16_wino_workspace_bytes(desc); launches on different streams need different workspaces).
 *   ct_conv_bf16_wino_supported   pure host: 1 only for 3x3 / stride 1 / pad 1 / dilation 1, cin % 8 == 0, cin >= 16, oh x ow = h x w,
 *                                 nseg == 0, res == NULL, lo == NULL.
 *   in_absmax    NULL: the entry point takes the maxima itself (ct_absmax_bf16_nhwc into the workspace); otherwise ANY valid upper
 *                bound per image (results stay within the mode's error bound for bounds up to 2^10 x the maximum).
 *   out_absmax   max |y| of what the launch stores for image n (the bf16 values), folded into line n (atomic max).
 * Any finite bf16 magnitude of the activations works (3e5 and 1e-6 alike); an all-zero image gives act(shift) exactly; an image's
 * bits never depend on its batch mates.  The forward entry point refuses (message in ct_last_error_string) unsupported
 * descriptors (CT_ERR_UNSUPPORTED), in / out buffers beyond 32-bit offsets (CT_ERR_UNSUPPORTED), slices that are not multiples of
 * 8 input channels (CT_ERR_INVALID) and a short workspace (CT_ERR_WORKSPACE). */
int ct_conv_bf16_wino_supported(const ct_conv_desc* d);
size_t ct_conv_bf16_wino_packed_bytes(int cin, int cout);
int ct_conv_pack_weights_bf16_wino(const float* const* w, const int* cout, int nparts, int cin, void* out, ct_stream_t stream);
size_t ct_conv_bf16_wino_workspace_bytes(const ct_conv_desc* d);
int ct_conv2d_bf16_wino_fwd(const ct_conv_desc* d, void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* max |x| per image over the channel slice [coff, coff + c) of an NHWC bf16 map [batch][hw][ctot]: CLEARS the `batch` lines
 * (CT_ABSMAX_LINE_BYTES each, the bit pattern of the fp32 value of the maximum in the first word) and then fills them. */
int ct_absmax_bf16_nhwc(const void* x, int batch, int hw, int ctot, int coff, int c, unsigned* lines, ct_stream_t stream);

/* ------------------------------------------------------------ training side ---- */
/* What `losses.backward()` (train.py:228) makes autograd/cuDNN do for the layers above.  The data
 * gradient of a convolution is ct_conv2d_fwd with desc.transposed = 1. */

/* Weight gradient of the convolution described by `d` (forward geometry; d->in = the forward input
 * X, d->wpacked/scale/shift/out unused):  dw[cout][cin][kh][kw] (dense fp32, overwritten) =
 * sum over batch and output pixels of dz[n][co][oh][ow] * X[n][ci][ih][iw];  dz is the channel slice
 * [dz_coff, dz_coff+cout) of an NCHW buffer with dz_ctot channels.  "Overwritten" holds for whatever dw contains on entry
 * (NaN included): the pixel splits add into dw after one memset inside the call.  Under ct_scratch_prezeroed(1) that
 * memset is the caller's, and the call ADDS the gradient to what dw holds.  The five weight-gradient entry points share their
 * argument checks: a null pointer (named in the message), a non-positive batch / cin / cout, an input slice outside d->in_ctot
 * (in_coff < 0 or in_coff + cin > in_ctot; this entry point did not check it before) or a dz slice outside dz_ctot is
 * CT_ERR_INVALID. */
int ct_conv2d_wgrad(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                    ct_stream_t stream);

/* The same weight gradient through Winograd F(3x3, 2x2) for 3x3 / stride 1 / dilation 1 / pad 1 layers
 * (2.25x fewer multiplications; same arguments and result layout as ct_conv2d_wgrad).  `workspace` holds
 * ct_conv_wgrad_wino_workspace_bytes(d) bytes (the 16 transform-domain partial sums [16][cout][cin]);
 * ct_conv_wgrad_wino_supported() tells whether the geometry qualifies (else CT_ERR_UNSUPPORTED). */
int ct_conv_wgrad_wino_supported(const ct_conv_desc* d);
size_t ct_conv_wgrad_wino_workspace_bytes(const ct_conv_desc* d);
int ct_conv2d_wgrad_wino(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                         void* workspace, ct_stream_t stream);
/* Winograd F(3x3, 4x4) weight gradient: the large-tile counterpart (4x4 dZ tiles, 6x6 input patches, 36 transform
 * points: 1.78x fewer multiplications than F(3x3, 2x2)), same contract; the workspace holds
 * ct_conv_wgrad_wino4_workspace_bytes(d) bytes ([36][cout][cin] partial sums). */
int ct_conv_wgrad_wino4_supported(const ct_conv_desc* d);
size_t ct_conv_wgrad_wino4_workspace_bytes(const ct_conv_desc* d);
int ct_conv2d_wgrad_wino4(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                          void* workspace, ct_stream_t stream);

/* The F(3x3, 4x4) weight gradient in the three-kernel form of ct_conv2d_wino4s_fwd (csrc/ct_wino4s.hip): dZ tiles and input
 * patches are transformed once (E = A e A^T, V = B^T d B), split exactly into three bfloat16 pieces and stored as MFMA operand
 * fragments with the TILE index as k; 36 GEMMs dU[xi][cout][cin] = sum_tiles E V^T on the bf16 matrix pipe (the forward form's
 * kernel, k split over several workgroups per block, one slab of dU per split, no atomics); a finishing kernel adds the slabs
 * in order and applies G^T . G.  Same arguments and result as ct_conv2d_wgrad_wino4 (train.py:228: autograd's conv
 * backward-weight for the wide 3x3 layers of models/RFB_Net_vgg.py:219-227,238-248); cin % 16 == 0; the workspace holds
 * ct_conv_wgrad_wino4s_workspace_bytes(d) bytes (E, V and the dU slabs). */
int ct_conv_wgrad_wino4s_supported(const ct_conv_desc* d);
size_t ct_conv_wgrad_wino4s_workspace_bytes(const ct_conv_desc* d);
int ct_conv2d_wgrad_wino4s(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                           void* workspace, size_t workspace_bytes, ct_stream_t stream);

/* The weight gradient of a 1x1 convolution (pad 0, dilation 1, stride 1 or 2) as ONE GEMM on the f16 matrix pipe in the f16x2
 * operand form (csrc/ct_wgrad_h2.hip, csrc/ct_f16x2.h): dw[cout][cin] = sum over batch and output pixels of dz * X, fp32
 * accumulation.  Arguments and result as ct_conv2d_wgrad; dw is OVERWRITTEN (no pre-zeroing).  The sum runs over the whole
 * batch, so each operand is scaled by ONE power of two per launch, from the maximum over the `batch` lines of d->in_absmax
 * (X) and dz_absmax (dZ); either may be NULL, the entry point then takes that maximum itself (a pass of ct_absmax_f32 into the
 * workspace, which may hold anything on entry).  A bound above the true maximum is valid.  Deterministic: k is split over
 * workgroups in a partition that depends on the descriptor alone, every split writes its own slab of the workspace and a
 * finishing kernel adds them in order -- no atomics, two calls on the same inputs give the same bits.  The workspace holds
 * ct_conv_wgrad_h2_workspace_bytes(d) bytes (slabs and the two maxima lines); a smaller one is CT_ERR_WORKSPACE.  Other
 * geometries and buffers above 2 GiB: CT_ERR_UNSUPPORTED (ct_conv_wgrad_h2_supported() = 0; ct_conv2d_wgrad takes those). */
int ct_conv_wgrad_h2_supported(const ct_conv_desc* d);
size_t ct_conv_wgrad_h2_workspace_bytes(const ct_conv_desc* d);
int ct_conv2d_wgrad_h2(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, const unsigned* dz_absmax, float* dw,
                       void* workspace, size_t workspace_bytes, ct_stream_t stream);

/* ---- deterministic twins (`_det`): ordered sums in place of atomics --------------------------------------------------
 * ct_conv2d_wgrad, ct_conv2d_wgrad_wino, ct_conv2d_wgrad_wino4, the sliced BatchNorm reductions and the two dbias sums let
 * the partial results of several workgroups meet through floating-point atomics, so the order in which they land decides
 * the last bits.  A `_det` twin runs the SAME kernels over the SAME partition, but every workgroup STORES its partial result
 * into a slab of its own in a caller-provided workspace, and a finishing kernel adds the slabs of each output element in
 * slab-index order: same build, same environment, same inputs => same bits, whatever the scheduling.  Every slab element the
 * finish reads is written by its producer, so the workspace may hold anything on entry, nothing is memset, and
 * ct_scratch_prezeroed() has no bearing on these entries: the output is always OVERWRITTEN.  The partition stays a pure
 * function of the descriptor and the environment; the size queries are host code (no device needed) and return through
 * `partials` (may be NULL) how many partial sums meet in one output element of that launch.
 *
 * Arguments, result layout and refusals are those of the plain entry (the message names the `_det` entry), plus: a
 * workspace that is NULL or not 16-byte aligned (scratch: 8-byte) is CT_ERR_INVALID, one smaller than the launch needs is
 * CT_ERR_WORKSPACE.
 *
 * Direct kernel.  One launch per batch chunk of max_chunk images (all of them unless X or dZ exceeds 2 GiB).  For a chunk
 * of nb images, with Npix = nb*oh*ow, Ncols = cin*kh*kw, tiles = ceil(cout/64) * ceil(Ncols/64) and slots = 512
 * (CTDET_WGRAD_WGS; tile edge 128 under CTDET_WGRAD_TB=2 where cout >= 96 and Ncols >= 96):
 *     smax   = max(1, min(ceil(Npix/256), 4*slots / tiles))
 *     want   = the first sp in 1..smax whose fill  tiles*sp / (ceil(tiles*sp / slots) * slots)  reaches 0.92,
 *              else the sp of the largest fill (the smallest such sp)
 *     per    = ceil(ceil(Npix/64) / want)        blocks of 64 pixels per split
 *     splits = ceil(ceil(Npix/64) / per)
 * Workspace: slabs [splits][cout][Ncols] floats per chunk, the chunks' slabs appended in chunk order; partials = the sum of
 * `splits` over the chunks; bytes = partials * cout * Ncols * 4.  The queries take dZ as dense (dz_ctot == cout) when they
 * count batch chunks; the entry checks workspace_bytes against the dz_ctot it is given.  0 / partials 0: a NULL or
 * non-positive descriptor, an oh/ow that does not follow from the geometry, a filter size that is not built. */
size_t ct_conv_wgrad_det_workspace_bytes(const ct_conv_desc* d, int* partials);
int ct_conv2d_wgrad_det(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                        void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* Winograd twins.  Per chunk of nb images, with tile = 2 / 4, points = 16 / 36, block = 64 / 32 channels per workgroup side,
 * wgs = 256 / 512 (CTDET_WW_WGS / CTDET_W4W_WGS) for F(3x3, 2x2) / F(3x3, 4x4):
 *     chunks = ceil(nb * ceil(h/tile) * ceil(w/tile) / 8),   blocks = ceil(cout/block) * ceil(cin/block)
 *     want   = min(65535, max(1, min(chunks, wgs / blocks))),  per = ceil(chunks / want),  splits = ceil(chunks / per)
 * Workspace: slabs [splits][points][cout][cin] floats, appended in chunk order; the finish adds them in order and then applies
 * G^T . G.  bytes = partials * points * cout * cin * 4; 0 / partials 0 where ct_conv_wgrad_wino_supported() is 0. */
size_t ct_conv_wgrad_wino_det_workspace_bytes(const ct_conv_desc* d, int* partials);
int ct_conv2d_wgrad_wino_det(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                             void* workspace, size_t workspace_bytes, ct_stream_t stream);
size_t ct_conv_wgrad_wino4_det_workspace_bytes(const ct_conv_desc* d, int* partials);
int ct_conv2d_wgrad_wino4_det(const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, float* dw,
                              void* workspace, size_t workspace_bytes, ct_stream_t stream);
/* BatchNorm twins: slices = max(1, min(ceil(1024/channels), batch*hw / 2048)) (= partials), slice y stores its two sums as
 * doubles at scratch[y][2][channels] and the final kernel adds the slices in order.  With one slice the one-workgroup
 * reduction runs and scratch is not looked at.  The query returns 16 * max(channels, min(1023 + channels, channels *
 * max(1, batch*hw / 2048))) bytes: at least slices * 2 * channels doubles, and growing with batch and with channels (which
 * slices * channels does not).  0 for a non-positive argument.  Arguments as the plain entries, `scratch` followed by its size. */
size_t ct_bn_det_scratch_bytes(int batch, int channels, int hw, int* partials);
int ct_bn_train_stats_det(const float* z, int batch, int ctot, int coff, int channels, int hw,
                          float* mean, float* var, float momentum, float* running_mean, float* running_var,
                          void* scratch, size_t scratch_bytes, ct_stream_t stream);
int ct_bn_train_backward_det(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                             const float* z, const float* mean, const float* var, const float* gamma,
                             float eps, int relu, const float* lo, float res_scale,
                             float* dres, int dres_ctot, int dres_coff, int dres_accumulate,
                             float* dz, float* dgamma, float* dbeta, int z_ctot, int z_coff,
                             int batch, int channels, int hw, void* scratch, size_t scratch_bytes, ct_stream_t stream);
int ct_bn_eval_backward_det(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                            const float* z, const float* running_mean, const float* running_var, const float* gamma,
                            float eps, int relu, const float* lo, float res_scale,
                            float* dres, int dres_ctot, int dres_coff, int dres_accumulate,
                            float* dz, float* dgamma, float* dbeta, int z_ctot, int z_coff,
                            int batch, int channels, int hw, void* scratch, size_t scratch_bytes, ct_stream_t stream);
/* dbias twins (arguments of ct_bias_act_backward_amax resp. ct_maxpool2x2_bias_relu_bwd, then scratch and its size; scratch is
 * looked at only where dbias is given).  Bias + activation: s0 = min(65535, max(1, min(ceil(2048/channels),
 * ceil(batch*hw / 4096)))), per = ceil(batch*hw / s0) rounded up to a multiple of 4, slices = ceil(batch*hw / per) (=
 * partials); slice y stores its sum as a double at scratch[y][channels].  The query returns 8 * max(channels, min(2047 +
 * channels, channels * ceil(batch*hw / 4096))) bytes (the same kind of bound as above).  Fused pool: one workgroup per
 * (image, channel) plane, so partials = batch and scratch holds [batch][channels] doubles, added in image order. */
size_t ct_bias_det_scratch_bytes(int batch, int channels, int hw, int* partials);
int ct_bias_act_backward_det(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                             int relu, int batch, int channels, int hw, float* dz, int dz_ctot, int dz_coff,
                             float* dbias, unsigned* dz_absmax, void* scratch, size_t scratch_bytes, ct_stream_t stream);
size_t ct_maxpool2x2_bias_relu_bwd_det_scratch_bytes(int batch, int channels, int* partials);
int ct_maxpool2x2_bias_relu_bwd_det(const float* y, int y_ctot, int y_coff, const float* dy, int batch, int channels, int h, int w,
                                    int oh, int ow, float* dz, int dz_ctot, int dz_coff, float* dbias, unsigned* dz_absmax,
                                    void* scratch, size_t scratch_bytes, ct_stream_t stream);

/* nn.BatchNorm2d(eps 1e-5, momentum 0.01) in training mode (models/RFB_Net_vgg.py:13,19), split in
 * three launches around the conv output z (channel slice [z_coff, z_coff+channels) of an NCHW buffer
 * with z_ctot channels; dz uses the same slicing):
 *   stats    per-channel batch mean / biased variance (+ running-stat update with the unbiased
 *            variance when running_mean/var are given)
 *   apply    y = act( ((z-mean)/sqrt(var+eps)*gamma + beta) [* res_scale + res] ) into a channel slice
 *   backward dz, dgamma, dbeta (and the residual branch's gradient) from dy */
/* `scratch` (both BatchNorm entry points): optional device buffer of 2*channels doubles; with it the per-channel
 * reductions are split over several workgroups per channel (f64 atomics), without it one workgroup per channel.
 * A call that splits (batch*hw >= 4096 and channels < 1024) leaves its two per-channel sums in scratch ([0, channels):
 * sum z resp. dbeta, [channels, 2*channels): sum z*z resp. dgamma, as doubles); it does NOT return scratch to zero, so
 * under ct_scratch_prezeroed(1) the caller zeroes a scratch buffer again before every call that uses it
 * (ctdet/train_engine.py: one buffer per layer, one memset of the arena before each pass).  A call that does not
 * split neither reads nor writes scratch. */
int ct_bn_train_stats(const float* z, int batch, int ctot, int coff, int channels, int hw,
                      float* mean, float* var, float momentum, float* running_mean, float* running_var,
                      void* scratch, ct_stream_t stream);
int ct_bn_train_apply(const float* z, const float* mean, const float* var, const float* gamma,
                      const float* beta, float eps, int relu, const float* lo, const float* res,
                      int res_ctot, int res_coff, float res_scale, float* y, int y_ctot, int y_coff,
                      int z_ctot, int z_coff, int batch, int channels, int hw, ct_stream_t stream);
int ct_bn_train_backward(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                         const float* z, const float* mean, const float* var, const float* gamma,
                         float eps, int relu, const float* lo, float res_scale,
                         float* dres, int dres_ctot, int dres_coff, int dres_accumulate,
                         float* dz, float* dgamma, float* dbeta, int z_ctot, int z_coff,
                         int batch, int channels, int hw, void* scratch, ct_stream_t stream);
/* The same backward for an nn.BatchNorm2d that sits in eval() mode inside a training network (frozen
 * statistics: ct_bn_train_apply was given running_mean / running_var): mean and variance are constants, so
 * dz = gamma / sqrt(var+eps) * dy_masked, dgamma = sum dy_masked * xhat, dbeta = sum dy_masked. */
int ct_bn_eval_backward(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                        const float* z, const float* running_mean, const float* running_var, const float* gamma,
                        float eps, int relu, const float* lo, float res_scale,
                        float* dres, int dres_ctot, int dres_coff, int dres_accumulate,
                        float* dz, float* dgamma, float* dbeta, int z_ctot, int z_coff,
                        int batch, int channels, int hw, void* scratch, ct_stream_t stream);
/* Synchronized BatchNorm (data-parallel training: statistics over the GLOBAL batch).  Each pass of a layer is split in three:
 * a local entry leaves the shard's two per-channel sums as doubles at sums[2][channels], the caller adds `sums` over the ranks
 * (one SUM all-reduce), and a second entry finishes from the reduced sums and count = global batch * hw.
 *   stats_local     sums = sum z, then sum z*z, over the shard's batch*hw elements of each channel
 *   stats_finish    m = S0/count, mean = (float)m, var = (float)max(S1/count - m*m, 0), running statistics with the float
 *                   unbias = count/(count-1) (1 for count <= 1): the expressions of ct_bn_train_stats
 *   backward_local  sums = sum g, then sum g*xhat, with g = masked dy * res_scale and xhat = (z - mean) / sqrt(var + eps) from
 *                   the GLOBAL mean / var; dbeta = (float)sum g and dgamma = (float)sum g*xhat of the shard (the gradient
 *                   all-reduce averages them like every other parameter gradient)
 *   backward_apply  dz and dres of ct_bn_train_backward, with (float)sums[c], (float)sums[channels + c] and (float)count in
 *                   place of dbeta[c], dgamma[c] and batch*hw
 * The local entries are ordered reductions: walk, slice rule, slice order and scratch (ct_bn_det_scratch_bytes) of the `_det`
 * twins, no floating-point atomics, no memset; one shard with count = batch*hw reproduces the twins bit for bit.  Refused with
 * CT_ERR_INVALID before any HIP call: a null pointer (dres, lo, y without a mask, the running statistics and a scratch that
 * one slice does not need may be null), a non-positive size, a count that is not finite and >= 1, a misaligned scratch, a null
 * scratch where slices > 1; CT_ERR_WORKSPACE: a scratch smaller than slices * 2 * channels doubles. */
int ct_bn_sync_stats_local(const float* z, int batch, int ctot, int coff, int channels, int hw, double* sums,
                           void* scratch, size_t scratch_bytes, ct_stream_t stream);
int ct_bn_sync_stats_finish(const double* sums, double count, int channels, float* mean, float* var, float momentum,
                            float* running_mean, float* running_var, ct_stream_t stream);
int ct_bn_sync_backward_local(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                              const float* z, const float* mean, const float* var, float eps, int relu, const float* lo,
                              float res_scale, int z_ctot, int z_coff, int batch, int channels, int hw,
                              double* sums, float* dgamma, float* dbeta, void* scratch, size_t scratch_bytes,
                              ct_stream_t stream);
int ct_bn_sync_backward_apply(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                              const float* z, const float* mean, const float* var, const float* gamma, float eps,
                              int relu, const float* lo, float res_scale, float* dres, int dres_ctot, int dres_coff,
                              int dres_accumulate, float* dz, int z_ctot, int z_coff, int batch, int channels, int hw,
                              const double* sums, double count, ct_stream_t stream);
/* y = act(conv + bias): dz = dy * (y > 0 if relu) into a channel slice, dbias[c] = sum dz (may be NULL). */
int ct_bias_act_backward(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                         int relu, int batch, int channels, int hw, float* dz, int dz_ctot, int dz_coff,
                         float* dbias, ct_stream_t stream);
/* The same, and max |dz| per image folded into dz_absmax (lines as ct_conv_desc.out_absmax; NULL = off): dz is the INPUT of the
 * layer's data-gradient convolution, whose f16x2 form takes its exponent from these maxima (train.py:222-229 backward). */
int ct_bias_act_backward_amax(const float* dy, int dy_ctot, int dy_coff, const float* y, int y_ctot, int y_coff,
                              int relu, int batch, int channels, int hw, float* dz, int dz_ctot, int dz_coff,
                              float* dbias, unsigned* dz_absmax, ct_stream_t stream);
/* MaxPool2d(2, 2) backward and the bias + ReLU backward of the convolution under the pool in one pass (train.py:222-229 backward of
 * models/RFB_Net_vgg.py:323-336 conv + ReLU + 'M'): y = the convolution's (post-ReLU) output = the pool's input, dy = the gradient
 * of the POOLED map [batch][channels][oh*ow]; writes dz = (y > 0) * (first maximum of its window) * dy into a channel slice,
 * dbias[c] += sum dz (NULL = skip), max |dz| per image into dz_absmax (NULL = off).  For a convolution whose output only the pool reads. */
int ct_maxpool2x2_bias_relu_bwd(const float* y, int y_ctot, int y_coff, const float* dy, int batch, int channels, int h, int w,
                                int oh, int ow, float* dz, int dz_ctot, int dz_coff, float* dbias, unsigned* dz_absmax,
                                ct_stream_t stream);
/* max_pool2d backward: the gradient goes to the first maximum of each window (torch's rule). */
int ct_maxpool2d_bwd(const float* x, const float* dy, float* dx, long planes, int h, int w, int oh, int ow,
                     int k, int stride, int pad, int accumulate, ct_stream_t stream);
/* Gradient of the channels-last head scatter (models/RFB_Net_vgg.py:239-248 permute/view/cat):
 * dz[n][co][pix] gathered from the flattened loc/conf/obj gradient buffers described by segs. */
int ct_head_grad_gather(const ct_out_segment* segs, int nseg, int batch, int channels, int hw,
                        float* dz, ct_stream_t stream);

/* Test-time input transform, data/data_augment.py:224-266 (BaseTransform.__call__): bilinear
 * cv2.resize of uint8 HxWx3 images to size x size, float32, minus `means3`, HWC -> CHW.
 * src holds `batch` images back to back; image n starts at src + offsets[n] and is
 * hw[2n] x hw[2n+1] x 3 bytes (offsets, hw: device arrays).  out = float [batch][3][size][size].
 * Integer arithmetic follows OpenCV's 8-bit INTER_LINEAR path (11-bit coefficients). */
int ct_preproc_resize(const unsigned char* src, const long long* offsets, const int* hw, int batch,
                      int size, const float* means3, float* out, ct_stream_t stream);

/* Training-time augmentation, data/data_augment.py:164-221 (`preproc.__call__`): crop -> photometric distortion
 * (8-bit HSV space) -> expand on a mean-filled canvas -> mirror -> resize -> minus means -> CHW, one gather launch
 * per batch.  `plans` = device array of `batch` records, typedef ct_aug_plan_record below (source offset / size, crop
 * rectangle, canvas size and placement, mirror flag, interpolation 0 linear / 1 nearest / 2 area, distortion flags
 * 1 brightness 2 contrast 4 hue 8 saturation with their parameters, canvas fill) holding the random DECISIONS the
 * host logic drew like the reference does.  Pixel arithmetic restates OpenCV's published 8-bit formulas (cv2 is
 * not in this image): tolerance-based parity. */
int ct_preproc_augment(const unsigned char* src, const void* plans, int batch, int size, const float* means3,
                       float* out, ct_stream_t stream);

/* One output coordinate of a separable fixed-point resize filter: source index of its first tap and the 11-bit
 * coefficients (2048 = 1.0) of taps first, first + 1, ...  The 4-tap filter uses c[0..3], the rest 0. */
typedef struct { int first; short c[8]; } ct_resize_tap;   /* 20 bytes */

/* ct_preproc_augment plus the two filters cv2.resize draws besides linear / nearest / area: plan.interp 3 =
 * bicubic (4 taps), 4 = Lanczos4 (8 taps), as OpenCV's 8-bit path computes them -- two separable passes in int32:
 *   h[r][d] = sum_j cx[d][j] * P(ix[d][j], r),   v = sum_j cy[d][j] * h[iy[d][j]][.],
 *   pixel = clamp((v + 2^21) >> 22, 0, 255), then minus mean, CHW,
 * P being the image that enters the resize (crop, distortion, canvas, mirror: the plan, unchanged layout).
 * `taps` = device array of batch * 2 * size records, image n's at taps + n*2*size: `size` records for x, then
 * `size` for y.  They are host decisions like the plan (ctdet/ops.py resize_taps: the Lanczos4 coefficients need a
 * double sin / cos that host and device round differently); the device does integer work only, so its pixels are
 * bit-reproducible.
 * SAFETY RULE: `first` is stored unclamped (floor(f) - (k/2 - 1)); the KERNEL clamps first + j to [0, n-1] of the
 * canvas before every read, so no table content can make it read outside the image -- this entry cannot inspect
 * device tables, the clamp is what makes foreign tables memory-safe.
 * Results are defined only for tables whose rows keep |v| inside int32; those of the two filters do (positive taps
 * of a row sum to <= 2780, |v| <= 255 * 2780^2 < 2^31).  Foreign tables are memory-safe but otherwise unspecified.
 * Images with interp 0..2 ignore their tables and come out bit-identical to ct_preproc_augment on the same plans
 * (one device function serves both kernels); ct_preproc_augment itself keeps treating unknown interp values as
 * linear.  Two forms of the same integer sums, chosen per workgroup: the source window of a 32x8 output tile
 * staged once in LDS when it fits, a per-pixel gather otherwise; CTDET_AUG_TILED=0 (read once per process) forces
 * the gather form everywhere.  They agree bit for bit. */
int ct_preproc_augment_taps(const unsigned char* src, const void* plans, const ct_resize_tap* taps, int batch,
                            int size, const float* means3, float* out, ct_stream_t stream);

/* mixup of two image batches, data/voc0712.py:262: out = img1 * lambd[n] + img2 * (1 - lambd[n]). */
int ct_mixup_blend(const float* img1, const float* img2, const float* lambd, int batch, long per_image,
                   float* out, ct_stream_t stream);

/* The augmentation DECISIONS and box targets of data/data_augment.py `preproc.decide` on the device
 * (csrc/ct_aug_plan.hip; host twin ctdet/aug_plan_ref.py).  It writes the plan records ct_preproc_augment reads and the
 * packed truths / gt_off pair ct_match_batched reads, so nothing per sample is left on the host.
 *
 * GENERATOR  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85),
 *   key = (seed lo, seed hi), counter = (sample_id lo, sample_id hi, slot, lane); one evaluation gives words w0..w3.
 *   A sample's decisions depend on (seed, sample_id, its H, W, boxes, cls) and nothing else.
 * DRAW RULES  uniform(a,b) = a + (b-a) * (w * 2^-32) in fp64; randrange(n) = (w * n) >> 32 on a 64-bit product;
 *   coin = w >> 31.  All decision arithmetic is fp64 with + - * / sqrt, comparisons, min/max and truncation only,
 *   contraction off, so host twin and device round alike.
 * DRAW TABLE
 *   slot        lane    w0                  w1               w2                   w3
 *   0           0       brightness coin     contrast coin    hue coin             saturation coin
 *   0           1       beta U(-32,32)      alpha U(.5,1.5)  hue -18 + rr(37)     sat U(.5,1.5)
 *   0           2       expand u            mirror coin      interp rr(5)         fallback interp rr(5)
 *   0x100 + r   63      crop mode rr(7)
 *   0x100 + r   0..49   scale U(.3,1)       ratio u          left rr(W - w)       top rr(H - h)
 *   0x200 + r   0..63   scale U(1,4)        ratio u          left rr(w - cw + 1)  top rr(h - ch + 1)
 * CROP (reference _crop)  no boxes: no crop.  Rounds r = 0..255: mode = CROP_MODES[rr(7)]; mode None ends the rounds
 *   without a crop; else the 50 lanes are the round's trials: ratio = sqrt(U(max(.5, scale^2), min(2, 1/scale/scale))),
 *   w = int(scale*ratio*W), h = int(scale/ratio*H).  A trial is rejected when w < 1, h < 1, w >= W or h >= H (the
 *   reference raises there: the one defined departure), when the mode's IoU condition fails (matrix_iou, min and max
 *   over the boxes), when no box centre lies strictly inside, or when cls >= 0 and no inside box is labelled cls + 1.
 *   The lowest passing lane wins; none: next round; after 256 rounds no crop.  Same distribution as the reference's
 *   sequential trials up to the cap's mass of at most (6/7)^256.
 * DISTORT  a parameter is used only when its coin is set.  EXPAND (on the crop, cw x ch)  taken unless u > p; rounds
 *   r = 0..63 of 64 trials: ratio = sqrt(U(max(.5, 1/scale/scale), min(2, scale^2))), ws = scale*ratio,
 *   hs = scale/ratio, rejected when ws < 1 or hs < 1, canvas int(ws*cw) x int(hs*ch); after 64 rounds no expand.
 * TARGETS  boxes whose centre is inside the crop, clipped to it and shifted; shifted by the canvas placement;
 *   mirrored (x1' = width - x2, x2' = width - x1); divided by the canvas size; rows with min(w, h) > 0.01 are kept.
 *   Nothing kept, or cls >= 0 and none of the kept rows labelled cls + 1: the identity plan, interp from the fallback
 *   word, and the original boxes divided by (W, H), unfiltered.  Rows are float32 [x1,y1,x2,y2,label,weight].
 *
 * SAFETY RULE (this entry cannot inspect device tables): box_begin / box_end are clamped to [0, total_boxes]; boxes
 * past max_gt of a sample are ignored; a sample whose image is outside [0, num_images) or below the largest in-range
 * image index of the samples before it, or whose H or W is below 1, gets the identity plan (of max(H,1) x max(W,1),
 * interp 0) and no rows, and sets status bit 1; rows past truths_cap are dropped (gt_off_out is capped with them) and
 * set status bit 2.  status = {bits, refused samples, dropped rows, rows before the cap}.  Nothing is written outside
 * the given sizes; every crop lies inside its image by construction.
 * Two launches, no allocation, no host synchronisation, capturable.  An image's rows are those of its samples in
 * sample order, in input order within a sample (what data_augment.mixup_targets gives). */
typedef struct {
    long long src_off;            /* byte offset of the sample's image in the Augmenter's source buffer; copied into the plan */
    unsigned long long sample_id;
    int H, W;
    int box_begin, box_end;       /* rows of `boxes` that belong to this sample */
    int image;                    /* the batch image its rows are appended to (non-decreasing over samples) */
    int cls;                      /* -1 or the few-shot class constraint of preproc.__call__ */
    float weight;                 /* column 6 of its rows (the mixup lambda, or 1) */
    int flags;                    /* 1: rows labelled -1 get weight 0 (voc0712.py:271-273)
                                     2: labels of the kept rows after the first become -1 (voc0712.py:237-238) */
} ct_aug_sample;                  /* 48 bytes */

/* One image's augmentation decisions: what ct_aug_plan writes per sample and every ct_preproc_augment* entry reads
 * (their `plans` arguments are arrays of these; the Python twins are in ctdet/aug_records.py). */
typedef struct {
    long long src_off;                        /* byte offset of the HxWx3 uint8 source image */
    int H, W;
    int crop_l, crop_t, crop_w, crop_h;
    int exp_w, exp_h, exp_left, exp_top;      /* canvas size (= crop size when not expanded) and placement */
    int mirror, interp;                       /* interp: 0 linear, 1 nearest, 2 area; 3 bicubic, 4 Lanczos4 (taps entry only) */
    int flags, hue_delta;                     /* flags: 1 brightness, 2 contrast, 4 hue, 8 saturation */
    float beta, alpha, sat_alpha;
    float fill[3];
    float pad0, pad1;
} ct_aug_plan_record;             /* 96 bytes */

size_t ct_aug_plan_workspace_bytes(int num_samples, int max_gt);
int ct_aug_plan(const ct_aug_sample* samples,   /* device array [num_samples] */
                int num_samples,
                const float* boxes,             /* device, [total_boxes,5] pixel x1,y1,x2,y2,label (finite) */
                int total_boxes,
                int num_images,
                int max_gt,                     /* boxes per sample the kernel looks at */
                unsigned long long seed,
                float p_expand,
                const int* interp_of_draw5,     /* host array */
                const float* fill3,             /* host array */
                void* plans_out,                /* device, ct_aug_plan_record [num_samples] */
                float* truths_out,              /* device, [truths_cap,6] */
                int truths_cap,
                int* gt_off_out,                /* device, [num_images+1] */
                int* status,                    /* device, [4] */
                void* workspace,
                size_t workspace_bytes,
                ct_stream_t stream);

/* MOSAIC: four samples composed into one size x size image (csrc/ct_aug_plan.hip, csrc/ct_preproc.hip; host twin
 * ctdet/aug_plan_ref.py mosaic_batch).  Opt-in; ct_aug_plan and ct_preproc_augment are untouched by it.
 *
 * SAMPLES  a batch of B images has 4B samples, group-major: sample s belongs to image s / 4 and sits in slot
 *   k = s % 4: 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right.
 * PER-SAMPLE DECISIONS  every sample gets the plan and the rows ct_aug_plan gives it: the draws, the crop / expand /
 *   mirror geometry, the cls constraint, the identity fallback and the flags / weight handling are unchanged and
 *   keyed by (seed, sample_id) and nothing else.
 * MEETING POINT  one Philox evaluation per image: key = seed, counter = (sample_id lo, sample_id hi, slot 0x300,
 *   lane 0) with the sample_id of the group's FIRST sample (slot 0x300 is outside the draw table above).
 *   cx = margin + randrange(S - 2*margin + 1) on w0, cy the same on w1; S = size, 1 <= margin <= S/2.
 * TILES (x0, y0, w, h; output pixels)  k0 (0, 0, cx, cy)  k1 (cx, 0, S-cx, cy)  k2 (0, cy, cx, S-cy)
 *   k3 (cx, cy, S-cx, S-cy).  They partition the square; every side is at least `margin`.
 * PIXELS (ct_preproc_augment_mosaic)  output pixel (x, y) of image i belongs to the lowest slot k whose tile has
 *   (unsigned)(x-x0) < (unsigned)w && (unsigned)(y-y0) < (unsigned)h.  Its value is what ct_preproc_augment computes
 *   for the plan of sample 4i+k at output coordinate (x-x0, y-y0) when the resize target is w x h instead of S x S:
 *   sx = (float)exp_w / w, sy = (float)exp_h / h; linear, nearest, area, area-when-enlarging taken as linear, unknown
 *   interp values as linear; then round, clamp, minus mean, CHW.  No tap filters (interp 3 / 4 run as linear).
 *   A tile with w < 1 or h < 1 is skipped; a pixel in no tile gets slot 0's canvas fill, (float)(int)fill[c] -
 *   means3[c].  These two rules only make foreign tile tables memory-safe: the planner produces neither case.
 * ROWS  a sample's rows are the float32 rows of its plan, normalised to its own canvas.  Each is mapped in fp64,
 *   rounded operation by operation: X1 = (x0 + (double)x1 * w) / S, X2 likewise, Y1 = (y0 + (double)y1 * h) / S, Y2
 *   likewise.  A row is kept when fmin(X2 - X1, Y2 - Y1) > 0.01 (the reference's rule, in units of the output image);
 *   label and weight pass through; kept rows are float32 [X1, Y1, X2, Y2, label, weight].  FALLBACK: an image with
 *   mapped rows of which none passes keeps all its mapped rows, unfiltered, so an image loses its targets only when
 *   all four samples were refused or had none.  An image's rows are those of its samples in slot order, in the
 *   planner's order within a sample.  gt_off_out, truths_cap and status keep their ct_aug_plan meaning.
 * SAFETY RULE (this entry cannot inspect device tables)  a sample whose `image` field is not s / 4, or whose H or W
 *   is below 1, is refused as in ct_aug_plan: identity plan, no rows, status bit 1; its tile is still rendered from
 *   that identity plan.  box_begin / box_end are clamped; nothing is written outside the given sizes.
 * INDEPENDENCE  an image's plans, tiles, rows and pixels depend on its own four samples and the seed only.
 * Three launches (plan, mosaic, pack) and one (render); no allocation, no host synchronisation, no H2D copy,
 * capturable.  CT_ERR_INVALID before any device work: null pointers, num_images < 1, max_gt < 1, size < 2, margin
 * outside 1..size/2, a workspace that is too small or not 16-byte aligned. */
typedef struct { int x0, y0, w, h; } ct_mosaic_tile;            /* 16 bytes */
size_t ct_aug_plan_mosaic_workspace_bytes(int num_images, int max_gt);
int ct_aug_plan_mosaic(const ct_aug_sample* samples /* dev [4*num_images] */, int num_images,
                       const float* boxes, int total_boxes, int max_gt, unsigned long long seed, float p_expand,
                       const int* interp_of_draw5, const float* fill3, int size, int margin,
                       void* plans_out /* dev, 4*num_images x 96 B */, ct_mosaic_tile* tiles_out /* dev [4*num_images] */,
                       float* truths_out, int truths_cap, int* gt_off_out, int* status,
                       void* workspace, size_t workspace_bytes, ct_stream_t stream);
int ct_preproc_augment_mosaic(const unsigned char* src, const void* plans, const ct_mosaic_tile* tiles,
                              int num_images, int size, const float* means3, float* out, ct_stream_t stream);

/* RANDOM AFFINE: a rotation, an isotropic scale, a shear and a shift of a rendered batch, with its rows carried along
 * (csrc/ct_affine.hip; host twin ctdet/aug_plan_ref.py affine_batch / warp_affine).  A post-stage on what the
 * renderers above produce -- float32 [B,3,S,S], mean-subtracted, and the packed rows normalised to that image -- so
 * it composes with the plain path, the tap filters, mixup and mosaic, none of whose entries it touches.  Opt-in.
 *
 * NO TRIGONOMETRY  host and device round sin / cos differently (see ct_preproc_augment_taps), so the rotation is drawn
 *   as t = tan(angle / 2), uniform in [-rot_half_tan, rot_half_tan], and the shear as its tangent; the caller computes
 *   the two bounds once.  cos = (1 - t^2) / (1 + t^2), sin = 2t / (1 + t^2): + - * / only.
 * GENERATOR  Philox4x32-10 and the draw rules of ct_aug_plan; key = seed, counter = (image id lo, image id hi, slot
 *   0x400, lane): a slot outside the draw table and the mosaic's 0x300.  uniform(a,b) = a + (b - a) * (w * 2^-32).
 *   lane 0   w0 t = uniform(-rot_half_tan, rot_half_tan)    w1 s = uniform(scale_lo, scale_hi)
 *            w2 kx = uniform(-shear_tan, shear_tan)         w3 ky likewise
 *   lane 1   w0 tx = uniform(0.5 - translate, 0.5 + translate) * S    w1 ty likewise
 *            w2 gate: w2 * 2^-32 > (double)p means the image is not warped
 * MATRIX  fp64, every operation rounded separately (contraction off), in this order:
 *     q = 1 + t*t;  c = (1 - t*t)/q;  n = (t + t)/q;  a = s*c;  b = s*n
 *     l00 = a - kx*b;  l01 = b + kx*a;  l10 = ky*a - b;  l11 = ky*b + a             shear . (rotation . scale)
 *     h = S*0.5
 *     fwd = {l00, l01, tx - (l00*h + l01*h),  l10, l11, ty - (l10*h + l11*h)}       about the centre, then the shift
 *     det = l00*l11 - l01*l10                     = s^2 (1 - kx ky) >= 0.75 s^2 by the bounds of the parameters
 *     i00 = l11/det;  i01 = -l01/det;  i10 = -l10/det;  i11 = l00/det
 *     inv = {i00, i01, -(i00*fwd2 + i01*fwd5),  i10, i11, -(i10*fwd2 + i11*fwd5)}
 * ROWS (ct_aug_affine_plan)  each row of the image, fp64: the corners (x1,y1) (x2,y1) (x1,y2) (x2,y2), each float32
 *   coordinate widened and multiplied by S; each corner through fwd as X = (fwd0*u + fwd1*v) + fwd2, Y = (fwd3*u +
 *   fwd4*v) + fwd5; the axis-aligned bounds by fmin / fmax in corner order; A0 = (X2 - X1)*(Y2 - Y1); every bound
 *   clipped as fmin(fmax(., 0), S); w = X2 - X1, h = Y2 - Y1 and A1 = w*h of the clipped bounds.  A row is kept when
 *   fmin(w, h)/S > (double)min_side && A1 >= (double)min_visible * A0, and is then float32 [X1/S, Y1/S, X2/S, Y2/S,
 *   label, weight]; label and weight pass through.  The box of a rotated box is its bounding box: targets grow with
 *   the angle (by a factor of at most |cos| + |sin| per side).
 *   GATE  an image the gate leaves alone gets the identity record, flags 4, and its rows unchanged, byte for byte.
 *   FALLBACK (the mosaic's rule)  an image that has rows of which none is kept is not warped: the identity record,
 *   flags 2|4, and its rows unchanged.  An applied image has flags 1.  The identity record is exactly fwd = inv =
 *   {1,0,0, 0,1,0}.
 *   Rows keep image order and input order within an image; they never outnumber the input's, so truths_rows, the
 *   capacity of BOTH row buffers, always suffices.  status = {bits, refused images, fallback images, rows out}.
 * SAFETY RULE (this entry cannot inspect device tables)  every gt_off_in value is clamped to [0, truths_rows].  An image
 *   whose clamped begin exceeds its clamped end, or lies below the clamped end of an image before it, is refused: the
 *   identity record (flags 4), no rows, status bit 1.  The images that remain read disjoint row ranges.  Nothing is
 *   written outside the given sizes.
 * INDEPENDENCE  an image's record and rows depend on (seed, its id, S, the parameters, its rows) and nothing else.
 * CT_ERR_INVALID before any device work: null pointers, batch < 1 or > 65535, size < 2 or > 16384, truths_rows < 0,
 *   a parameter that is not finite or outside the range its comment gives, row buffers that overlap, a workspace that
 *   is too small or not 16-byte aligned.  Two launches, no allocation, no host synchronisation, capturable.
 * PIXELS (ct_preproc_warp_affine)  output pixel (x, y) of image n, every channel c:
 *     X = ((double)inv0*x + (double)inv1*y) + inv2;  Y = ((double)inv3*x + (double)inv4*y) + inv5      fp64, op by op
 *     unless -1 < X && X < S && -1 < Y && Y < S (false for NaN) the pixel is border3[c] and no index is formed
 *     ix = floor(X); fx = (float)(X - ix);  iy, fy likewise
 *     tap(jx, jy) = in[n][c][jy][jx] when 0 <= jx < S and 0 <= jy < S, else border3[c]         constant border, blended
 *     a = tap(ix, iy), b = tap(ix+1, iy), cc = tap(ix, iy+1), d = tap(ix+1, iy+1)
 *     top = a + fx*(b - a);  bot = cc + fx*(d - cc);  pixel = top + fy*(bot - top)             fp32, op by op, no fma
 *   A record with flag 4 copies its image; the rule above gives the same bits for the identity matrix (fx = fy = 0),
 *   so the copy is a shortcut and not a second definition.  The outside rule and the per-tap test make ANY record table
 *   memory-safe: NaN, infinite or huge matrices yield border pixels.  `in` and `out` must not overlap
 *   (CT_ERR_INVALID).  One launch: a 32x8 output tile per 256-thread workgroup, one thread per pixel for the three
 *   channels; no allocation, no host synchronisation, capturable. */
typedef struct {
    double fwd[6];   /* source pixel (u,v) -> output pixel: x = fwd0*u + fwd1*v + fwd2, y = fwd3*u + fwd4*v + fwd5 */
    double inv[6];   /* output pixel -> source pixel */
    int flags;       /* 1 drawn and applied; 2 fallback (rows would all have been lost); 4 identity: the warp copies */
    int pad;
} ct_affine_record;  /* 104 bytes */

typedef struct {
    double rot_half_tan;       /* tan(max angle / 2), 0..1 */
    double scale_lo, scale_hi; /* 0 < lo <= hi <= 4 */
    double shear_tan;          /* tan(max shear), 0..0.5 */
    double translate;          /* fraction of S, 0..0.5 */
    float p;                   /* probability that an image is warped, 0..1 */
    float min_side;            /* rows kept when min(w,h) > min_side (normalised; the pipeline's 0.01), 0..1 */
    float min_visible;         /* and when clipped area >= min_visible * unclipped area, 0..1 */
} ct_affine_params;            /* host struct */

size_t ct_aug_affine_plan_workspace_bytes(int batch, int truths_rows);
int ct_aug_affine_plan(const float* truths_in /* dev [truths_rows,6] */, const int* gt_off_in /* dev [batch+1] */,
                       const unsigned long long* image_ids /* dev [batch] */, int batch, int truths_rows, int size,
                       unsigned long long seed, const ct_affine_params* params /* host */,
                       ct_affine_record* records_out /* dev [batch] */, float* truths_out /* dev [truths_rows,6] */,
                       int* gt_off_out /* dev [batch+1] */, int* status /* dev [4] */, void* workspace,
                       size_t workspace_bytes, ct_stream_t stream);
int ct_preproc_warp_affine(const float* in /* dev [batch,3,size,size] */, const ct_affine_record* records /* dev [batch] */,
                           int batch, int size, const float* border3 /* host */, float* out, ct_stream_t stream);

/* torch.nn.MaxPool2d of models/RFB_Net_vgg.py:328-330,338 (2x2 s2 [ceil], 3x3 s1 p1) on an NCHW
 * buffer: planes = batch*channels; windows are clipped to the input (ceil_mode semantics are
 * encoded in oh/ow by the caller). */
int ct_maxpool2d_fwd(const float* in, float* out, long planes, int h, int w, int oh, int ow,
                     int k, int stride, int pad, ct_stream_t stream);
/* Context pooling of models/RFB_Net_vgg.py:243-244 on the channels-last head output:
 * in  = conf logits of one source, per image [h*w, ch] at in + n*in_img_stride
 * out = max_pool2d(k, stride k, ceil_mode) -> [oh*ow, ch] at out + n*out_img_stride */
int ct_ctx_pool_fwd(const float* in, long long in_img_stride, float* out, long long out_img_stride,
                    int batch, int h, int w, int ch, int k, ct_stream_t stream);

/* ------------------------------------------------ Context-Transformer block ---- */

/* models/RFB_Net_vgg.py:253-271 fused (flash-style, W never materialised):
 *   theta = Lin_t(conf)+conf; phi = Lin_p(pool)+pool; g = Lin_g(pool)+pool
 *   delta = softmax(theta phi^T, dim=2) g * Wz;  nov = normalize(conf+delta) OBJ^T * scale
 *   setting 'incre' (fc_w != NULL): out = cat(Lin_fc(conf)+conf, nov)
 * conf dev [B,P,d], pool dev [B,M,d], out dev [B,P,(fc_w?d:0)+T]; d <= 64, T <= 32.
 * Linear weights are [d,d] row-major (out,in) as torch.nn.Linear stores them.
 * Both contractions carry their fp32 operands on the 16-bit matrix pipe: as three bfloat16 pieces / six products (default), or,
 * with CTDET_ATTN_H2=1 in the environment (read per call; round 6), as two binary16 pieces / three products (csrc/ct_f16x2.h: a
 * query row scaled by its own power of two, phi and g by one per image, the probabilities by 2^14) -- 1.2-1.34x faster, same error
 * against fp64, another rounding.  ct_ctx_attention_piece_products() returns the products per multiply-add in force (6 or 3);
 * ct_ctx_attention_fwd_train follows the same switch. */
typedef struct ct_ctx_params {
    const float *theta_w, *theta_b, *phi_w, *phi_b, *g_w, *g_b;
    const float *wz;          /* [d] */
    const float *obj_w;       /* [T,d] */
    const float *fc_w, *fc_b; /* optional ('incre'), [d,d],[d] */
    float scale;              /* the non-trainable `scale` parameter (5) */
    int d, t;
} ct_ctx_params;
size_t ct_ctx_attention_workspace_bytes(int batch, int num_priors, int num_ctx, int d);
int ct_ctx_attention_piece_products(void);
int ct_ctx_attention_fwd(const float* conf, const float* pool, int batch, int num_priors,
                         int num_ctx, const ct_ctx_params* prm, float* out,
                         void* workspace, size_t workspace_bytes, ct_stream_t stream);


/* ---- training of the Context-Transformer block ------------------------------------------------
 * The reference differentiates models/RFB_Net_vgg.py:253-271 with autograd (train.py:222-229).
 * Here: a forward that additionally saves, per query row, the aggregated context D = softmax(S) g
 * and the row log-sum-exp (`saved`, ct_ctx_attention_saved_bytes), and one backward entry point
 * that recomputes the affinity tiles on the MFMA path instead of storing the [P,M] matrix. */
size_t ct_ctx_attention_saved_bytes(int batch, int num_priors);
int ct_ctx_attention_fwd_train(const float* conf, const float* pool, int batch, int num_priors,
                               int num_ctx, const ct_ctx_params* prm, float* out, void* saved,
                               size_t saved_bytes, void* workspace, size_t workspace_bytes,
                               ct_stream_t stream);
/* Gradient buffers (device), same shapes as the parameters; overwritten by ct_ctx_attention_bwd. */
typedef struct ct_ctx_grads {
    float *theta_w, *theta_b, *phi_w, *phi_b, *g_w, *g_b;
    float *wz, *obj_w;
    float *fc_w, *fc_b;       /* required iff prm->fc_w */
} ct_ctx_grads;
size_t ct_ctx_attention_bwd_workspace_bytes(int batch, int num_priors, int num_ctx);
/* dout [B,P,(fc?d:0)+T] -> dconf [B,P,d] (direct + theta + fc_base paths; the pooled path is added
 * by ct_ctx_pool_bwd), dpool [B,M,d], parameter gradients in `grads`. */
int ct_ctx_attention_bwd(const float* conf, const float* pool, int batch, int num_priors, int num_ctx,
                         const ct_ctx_params* prm, const void* saved, const float* dout, float* dconf,
                         float* dpool, const ct_ctx_grads* grads, void* workspace,
                         size_t workspace_bytes, ct_stream_t stream);
/* The deterministic twin of ct_ctx_attention_bwd (the `_det` rules above: same kernels, same partition, stores in place of
 * atomics, the workspace may hold anything on entry, nothing is memset, every output is overwritten).  Arguments, results and
 * refusals are those of ct_ctx_attention_bwd; a workspace that is NULL or not 16-byte aligned is CT_ERR_INVALID, one smaller than
 * the query's answer CT_ERR_WORKSPACE.  With P_pad / M_pad = num_priors / num_ctx rounded up to 128, partial sums meet at four
 * sites; partials[] (may be NULL) reports how many per output element:
 *     [0] = ceil(P_pad / 256) * batch        the output pass: dwz [d], dobj [t][d]        (one per workgroup, 256 query rows)
 *     [1] = max(1, min(P_pad / 256, ceil(1024 / ((M_pad / 128) * batch))))                 the key side: dK, dV (kv_split)
 *     [2] = ceil(num_priors / 256) * batch   the query-side linears: theta, fc_base        (dW [d][d], db [d] per workgroup)
 *     [3] = ceil(num_ctx / 256) * batch      the key-side linears: phi, g
 * Workspace: the carve of ct_ctx_attention_bwd_workspace_bytes, then fp32 slabs, each area rounded up to 256 bytes:
 *     [partials[1]][batch][M_pad][64]        dV's slabs, then (stream order) dK's in the same area; absent when partials[1] == 1,
 *                                            the workgroups then store straight into dK / dV
 *     [partials[0]][(t + 1) * d]             dwz, dobj
 *     [partials[2]][(d + 1) * d]             theta; once more for fc_base when incre != 0
 *     [partials[3]][(d + 1) * d]             phi, and once more for g
 * Inside the output pass the 64 rows of a workgroup add their dwz terms in row order (no LDS atomics).  Order of the sums: dK / dV
 * element = slab 0 + slab 1 + ... in fp32, in slab order.  A small gradient whose slabs are [batch][nx] (workgroup x of image b
 * writes slab b * nx + x), in double, rounded once to fp32:
 *     s(b) = slab[b][0] + slab[b][1] + ... + slab[b][nx-1];   t(l) = s(l) + s(l + 8) + s(l + 16) + ...  (l = 0 .. 7);
 *     out  = t(0) + t(1) + ... + t(7)
 * -- a fixed tree that depends on (batch, nx) alone.  The query is host code; 0 (partials all 0) for a non-positive size, d outside
 * 1 .. 64 or t outside 1 .. 32. */
size_t ct_ctx_attention_bwd_det_workspace_bytes(int batch, int num_priors, int num_ctx, int d, int t, int incre, int partials[4]);
int ct_ctx_attention_bwd_det(const float* conf, const float* pool, int batch, int num_priors, int num_ctx,
                             const ct_ctx_params* prm, const void* saved, const float* dout, float* dconf,
                             float* dpool, const ct_ctx_grads* grads, void* workspace,
                             size_t workspace_bytes, ct_stream_t stream);
/* Backward of ct_ctx_pool_fwd (max_pool2d, kernel = stride = k, ceil_mode, channels-last): adds the
 * window gradient dpool to din at the first maximum of each window (torch's tie rule). */
int ct_ctx_pool_bwd(const float* in, long long in_img_stride, const float* dpool,
                    long long dpool_img_stride, float* din, long long din_img_stride, int batch,
                    int h, int w, int ch, int k, ct_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CTDET_H */
