// libctdet: host-side NMS entry points of the reference's `--cpu` path
// (utils/nms/cpu_nms.pyx:17-68 `cpu_nms`, :70-163 `cpu_soft_nms`).  These ARE the reference's
// CPU API (utils/nms_wrapper.py:27-30 `force_cpu`), not a fallback for the device kernels.
// Built with -ffp-contract=off so fp32 expressions round exactly like the Cython/C original.
#include "ct_common.h"
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

extern "C" int ct_cpu_nms(const float* dets, int n, float thresh, int ge, int* keep_out, int* num_out)
{
    CT_REQUIRE(num_out && (n == 0 || (dets && keep_out)) && n >= 0, "ct_cpu_nms: bad arguments");
    *num_out = 0;
    if (n == 0) return CT_OK;
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    // descending score, lower index first on ties (the build's defined tie order)
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return dets[(size_t)a * 5 + 4] > dets[(size_t)b * 5 + 4]; });
    std::vector<float> area(n);
    for (int i = 0; i < n; ++i) {
        const float* b = dets + (size_t)i * 5;
        area[i] = (b[2] - b[0] + 1.0f) * (b[3] - b[1] + 1.0f);
    }
    std::vector<unsigned char> dead(n, 0);
    int nk = 0;
    for (int _i = 0; _i < n; ++_i) {
        const int i = order[_i];
        if (dead[i]) continue;
        keep_out[nk++] = i;
        const float* a = dets + (size_t)i * 5;
        const float ix1 = a[0], iy1 = a[1], ix2 = a[2], iy2 = a[3], iarea = area[i];
        for (int _j = _i + 1; _j < n; ++_j) {
            const int j = order[_j];
            if (dead[j]) continue;
            const float* b = dets + (size_t)j * 5;
            const float xx1 = ix1 >= b[0] ? ix1 : b[0];
            const float yy1 = iy1 >= b[1] ? iy1 : b[1];
            const float xx2 = ix2 <= b[2] ? ix2 : b[2];
            const float yy2 = iy2 <= b[3] ? iy2 : b[3];
            const float w0 = xx2 - xx1 + 1.0f, h0 = yy2 - yy1 + 1.0f;
            const float w = 0.0f >= w0 ? 0.0f : w0;
            const float h = 0.0f >= h0 ? 0.0f : h0;
            const float inter = w * h;
            const float ovr = inter / (iarea + area[j] - inter);
            if (ge ? (ovr >= thresh) : (ovr > thresh)) dead[j] = 1;
        }
    }
    *num_out = nk;
    return CT_OK;
}

extern "C" int ct_cpu_soft_nms(float* boxes, int n, float sigma, float Nt, float threshold,
                               unsigned method, int* n_out)
{
    CT_REQUIRE(n_out && (n == 0 || boxes) && n >= 0, "ct_cpu_soft_nms: bad arguments");
    int N = n;
    auto B = [&](int r, int c) -> float& { return boxes[(size_t)r * 5 + c]; };
    for (int i = 0; i < N; ++i) {
        float maxscore = B(i, 4);
        int maxpos = i;
        float t[5];
        for (int c = 0; c < 5; ++c) t[c] = B(i, c);
        for (int pos = i + 1; pos < N; ++pos)
            if (maxscore < B(pos, 4)) {
                maxscore = B(pos, 4);
                maxpos = pos;
            }
        for (int c = 0; c < 5; ++c) B(i, c) = B(maxpos, c);
        for (int c = 0; c < 5; ++c) B(maxpos, c) = t[c];
        const float tx1 = B(i, 0), ty1 = B(i, 1), tx2 = B(i, 2), ty2 = B(i, 3);
        int pos = i + 1;
        while (pos < N) {
            const float x1 = B(pos, 0), y1 = B(pos, 1), x2 = B(pos, 2), y2 = B(pos, 3);
            const float area = (x2 - x1 + 1.0f) * (y2 - y1 + 1.0f);
            const float iw = std::min(tx2, x2) - std::max(tx1, x1) + 1.0f;
            if (iw > 0) {
                const float ih = std::min(ty2, y2) - std::max(ty1, y1) + 1.0f;
                if (ih > 0) {
                    const float ua = (tx2 - tx1 + 1.0f) * (ty2 - ty1 + 1.0f) + area - iw * ih;
                    const float ov = iw * ih / ua;
                    float weight;
                    if (method == 1) weight = ov > Nt ? 1.0f - ov : 1.0f;
                    else if (method == 2) weight = (float)std::exp(-((double)ov * (double)ov) / (double)sigma);
                    else weight = ov > Nt ? 0.0f : 1.0f;
                    B(pos, 4) = weight * B(pos, 4);
                    if (B(pos, 4) < threshold) {
                        for (int c = 0; c < 5; ++c) B(pos, c) = B(N - 1, c);
                        --N;
                        --pos;
                    }
                }
            }
            ++pos;
        }
    }
    *n_out = N;
    return CT_OK;
}

// The host twin of box_vote_kernel (ct_tta.hip) on one (image, class) segment: every output row's box becomes the
// weight-weighted mean of the candidates that overlap it by at least vote_thresh.  The fp32 IoU expression of ct_cpu_nms,
// float64 sums taken sequentially in candidate order, one float64 division, one rounding to fp32; a row without a member
// keeps its bits, and so does every score.
extern "C" int ct_cpu_box_vote(const float* cand_boxes, const float* weights, int n, float vote_thresh, float* rows, int m)
{
    CT_REQUIRE(n >= 0 && m >= 0 && (n == 0 || (cand_boxes && weights)) && (m == 0 || rows), "ct_cpu_box_vote: bad arguments");
    CT_REQUIRE(vote_thresh > 0.f && vote_thresh <= 1.f, "ct_cpu_box_vote: vote_thresh %g is outside (0, 1]", (double)vote_thresh);
    for (int r = 0; r < m; ++r) {
        float* t = rows + (size_t)r * 5;
        const float tx1 = t[0], ty1 = t[1], tx2 = t[2], ty2 = t[3];
        const float tarea = (tx2 - tx1 + 1.0f) * (ty2 - ty1 + 1.0f);
        double sw = 0.0, s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < n; ++j) {
            const float* b = cand_boxes + (size_t)j * 4;
            const float xx1 = tx1 >= b[0] ? tx1 : b[0];
            const float yy1 = ty1 >= b[1] ? ty1 : b[1];
            const float xx2 = tx2 <= b[2] ? tx2 : b[2];
            const float yy2 = ty2 <= b[3] ? ty2 : b[3];
            const float w0 = xx2 - xx1 + 1.0f, h0 = yy2 - yy1 + 1.0f;
            const float w = 0.0f >= w0 ? 0.0f : w0;
            const float h = 0.0f >= h0 ? 0.0f : h0;
            const float inter = w * h;
            const float area = (b[2] - b[0] + 1.0f) * (b[3] - b[1] + 1.0f);
            const float ovr = inter / (tarea + area - inter);
            if (ovr >= vote_thresh) {
                const double wq = (double)weights[j];
                sw += wq;
                for (int c = 0; c < 4; ++c) s[c] += wq * (double)b[c];
            }
        }
        if (sw > 0.0)
            for (int c = 0; c < 4; ++c) t[c] = (float)(s[c] / sw);
    }
    return CT_OK;
}

// The host twin of matrix_nms_segments_kernel (ct_matrix_nms.hip) on one (image, class) segment in the pipeline's order:
// the rule of include/ctdet.h as plain loops.  The fp32 IoU expression of ct_cpu_soft_nms; every term of the Gaussian
// method takes its own double exp.
extern "C" int ct_cpu_matrix_nms(const float* rows_sorted, int n, int method, float sigma, float score_threshold, int pre_top,
                                 int max_emit, float* out_rows, int* out_pos, int* n_out)
{
    CT_REQUIRE(n_out && n >= 0 && (n == 0 || (rows_sorted && out_rows && out_pos)), "ct_cpu_matrix_nms: bad arguments");
    CT_REQUIRE(method == 1 || method == 2, "ct_cpu_matrix_nms: method %d is not 1 (linear) or 2 (Gaussian)", method);
    CT_REQUIRE(method != 2 || sigma > 0.f, "ct_cpu_matrix_nms: sigma must be > 0 for the Gaussian method");
    CT_REQUIRE(pre_top > 0 && max_emit >= 0, "ct_cpu_matrix_nms: bad sizes (pre_top=%d max_emit=%d)", pre_top, max_emit);
    *n_out = 0;
    const int m = std::min(n, pre_top);
    if (m == 0) return CT_OK;
    auto R = [&](int r, int c) { return rows_sorted[(size_t)r * 5 + c]; };
    auto ov = [&](int i, int j) {
        const float iw = std::min(R(i, 2), R(j, 2)) - std::max(R(i, 0), R(j, 0)) + 1.0f;
        if (iw > 0) {
            const float ih = std::min(R(i, 3), R(j, 3)) - std::max(R(i, 1), R(j, 1)) + 1.0f;
            if (ih > 0) {
                const float area = (R(j, 2) - R(j, 0) + 1.0f) * (R(j, 3) - R(j, 1) + 1.0f);
                const float ua = (R(i, 2) - R(i, 0) + 1.0f) * (R(i, 3) - R(i, 1) + 1.0f) + area - iw * ih;
                return iw * ih / ua;
            }
        }
        return 0.0f;
    };
    std::vector<float> cmax(m, 0.0f), score(m);
    for (int j = 1; j < m; ++j)
        for (int k = 0; k < j; ++k) cmax[j] = std::max(cmax[j], ov(k, j));
    for (int j = 0; j < m; ++j) {
        float decay = 1.0f;
        for (int i = 0; i < j; ++i) {
            const float o = ov(i, j);
            float t;
            if (method == 1) {
                const float den = 1.0f - cmax[i];
                if (den == 0.0f) continue;
                t = (1.0f - o) / den;
            } else {
                t = (float)std::exp(((double)cmax[i] * (double)cmax[i] - (double)o * (double)o) / (double)sigma);
            }
            decay = std::min(decay, t);
        }
        score[j] = R(j, 4) * decay;
    }
    std::vector<int> order;
    for (int j = 0; j < m; ++j)
        if (!(score[j] < score_threshold)) order.push_back(j);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return score[a] > score[b]; });
    int k = 0;
    for (int j : order) {
        if (max_emit > 0 && k >= max_emit && score[j] != out_rows[(size_t)(k - 1) * 5 + 4]) break;
        for (int c = 0; c < 4; ++c) out_rows[(size_t)k * 5 + c] = R(j, c);
        out_rows[(size_t)k * 5 + 4] = score[j];
        out_pos[k++] = j;
    }
    *n_out = k;
    return CT_OK;
}
