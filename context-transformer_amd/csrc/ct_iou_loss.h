// The IoU-family localisation terms of the fused MultiBoxLoss (include/ctdet.h, ct_multibox_loss_fwd_loc): value and
// hand-derived gradient of one positive row, as functions of (loc, loc_t, prior, var0, var1) alone.  Plain fp32 with
// every operation rounded separately (the including file is compiled with -ffp-contract=off); host and device.
//
// A = decode(loc, prior) is the prediction, T = decode(loc_t, prior) the matched box.  The backward treats the loss
// as a function of eight quantities of A -- the corners x1 y1 x2 y2, the centre cx cy and the size w h -- and chains
//   x1 = cx - w/2, x2 = cx + w/2,  cx = pcx + l0 var0 pw,  w = pw exp(l2 var1)      (y likewise):
//   dL/dl0 = (g_x1 + g_x2 + g_cx) var0 pw,      dL/dl2 = ((g_x2 - g_x1)/2 + g_w) w var1.
// With I = inter, U = union, C = cw ch, c2 = cw^2 + ch^2, rho2 = centre distance^2, v = (4/pi^2) (atan T - atan A)^2:
//   corner q:  dI_q = +-(other side of the intersection) where q is the active argument of its min/max and iw, ih > 0;
//              dU_q = -dI_q, so d(1 - IoU)_q = -dI_q (1 + IoU) / U;
//              giou: + dI_q / C + U dC_q / C^2;     diou, ciou: - rho2 dc2_q / c2^2;
//   size w:    d(1 - IoU)_w = IoU h / U;   giou: - h / C;   ciou: + alpha dv_w, dv_w = -2 (4/pi^2) (atan T - atan A) h / (w^2 + h^2);
//   size h:    the same with w and h exchanged and dv_h = +2 (4/pi^2) (atan T - atan A) w / (w^2 + h^2);
//   centre:    diou, ciou: 2 (cx - tcx) / c2.
// alpha = v / ((1 - IoU) + v) is a constant in the backward (0 when v = 0).  At a kink (equal min/max arguments, iw or
// ih exactly 0) the strict comparisons below pick one of the one-sided derivatives.
#pragma once
#include "ctdet.h"

#if defined(__HIPCC__)
#define CT_IOU_HD __host__ __device__ __forceinline__
#else
#define CT_IOU_HD inline
#endif

namespace ctdet {

struct IouRow {
    float ax1, ay1, ax2, ay2, acx, acy, aw, ah;     // A
    float tx1, ty1, tx2, ty2, tcx, tcy;             // T
    float iw, ih, uni, iou, cw, ch;
    float rho2, c2;                                 // diou, ciou
    float dat, alpha;                               // ciou: atan(T.w/T.h) - atan(A.w/A.h), the constant alpha
    float loss;
};

constexpr float IOU_FOUR_OVER_PI2 = 0.40528473456935109f;

template <class F4>
CT_IOU_HD IouRow iou_row_forward(const F4& l, const F4& lt, const F4& p, float var0, float var1, int kind)
{
    IouRow r;
    r.acx = p.x + l.x * var0 * p.z;
    r.acy = p.y + l.y * var0 * p.w;
    r.aw = p.z * expf(l.z * var1);
    r.ah = p.w * expf(l.w * var1);
    r.tcx = p.x + lt.x * var0 * p.z;
    r.tcy = p.y + lt.y * var0 * p.w;
    const float tw = p.z * expf(lt.z * var1);
    const float th = p.w * expf(lt.w * var1);
    r.ax1 = r.acx - r.aw / 2.f; r.ay1 = r.acy - r.ah / 2.f;
    r.ax2 = r.acx + r.aw / 2.f; r.ay2 = r.acy + r.ah / 2.f;
    r.tx1 = r.tcx - tw / 2.f; r.ty1 = r.tcy - th / 2.f;
    r.tx2 = r.tcx + tw / 2.f; r.ty2 = r.tcy + th / 2.f;
    // Two intervals of widths wa, wt whose centres are d apart overlap by min(wa, wt, (wa + wt)/2 - d) and span
    // max(wa, wt, (wa + wt)/2 + d): the same iw, ih, cw, ch as from the corners, without subtracting coordinates that
    // are large against the box (and exactly w, h when A = T, where L is then exactly 0).  The corners serve the
    // backward's comparisons only.
    const float dcx = fabsf(r.acx - r.tcx), dcy = fabsf(r.acy - r.tcy);
    const float hw = (r.aw + tw) / 2.f, hh = (r.ah + th) / 2.f;
    r.iw = fmaxf(0.f, fminf(fminf(r.aw, tw), hw - dcx));
    r.ih = fmaxf(0.f, fminf(fminf(r.ah, th), hh - dcy));
    const float inter = r.iw * r.ih;
    r.uni = r.aw * r.ah + tw * th - inter;
    r.iou = inter / r.uni;
    r.cw = fmaxf(fmaxf(r.aw, tw), hw + dcx);
    r.ch = fmaxf(fmaxf(r.ah, th), hh + dcy);
    r.rho2 = r.c2 = r.dat = r.alpha = 0.f;
    float loss = 1.f - r.iou;
    if (kind == CT_LOC_GIOU) {
        const float ca = r.cw * r.ch;
        loss += (ca - r.uni) / ca;
    } else if (kind >= CT_LOC_DIOU) {
        r.rho2 = dcx * dcx + dcy * dcy;
        r.c2 = r.cw * r.cw + r.ch * r.ch;
        loss += r.rho2 / r.c2;
        if (kind == CT_LOC_CIOU) {
            r.dat = atanf(tw / th) - atanf(r.aw / r.ah);
            const float v = IOU_FOUR_OVER_PI2 * (r.dat * r.dat);
            r.alpha = v > 0.f ? v / ((1.f - r.iou) + v) : 0.f;
            loss += r.alpha * v;
        }
    }
    r.loss = loss;
    return r;
}

// d loss / d (l0, l1, l2, l3) of the row `r` came from, times `scale`
template <class F4>
CT_IOU_HD void iou_row_backward(const IouRow& r, const F4& p, float var0, float var1, int kind, float scale,
                                float& d0, float& d1, float& d2, float& d3)
{
    const float inv_u = 1.f / r.uni;
    const float k_iou = (1.f + r.iou) * inv_u;
    const float ca = r.cw * r.ch;
    const float inv_c = kind == CT_LOC_GIOU ? 1.f / ca : 0.f;
    const float k_c = kind == CT_LOC_GIOU ? r.uni * inv_c * inv_c : 0.f;                 // U / C^2
    const float k_c2 = kind >= CT_LOC_DIOU ? 2.f * r.rho2 / (r.c2 * r.c2) : 0.f;         // 2 rho2 / c2^2
    // one corner: dI = d inter, (dcw, dch) = d of the enclosing box's sides, each -1, 0 or +1 times the other side
    auto corner = [&](float dI, float dcw, float dch) -> float {
        float g = -(dI * k_iou);
        if (kind == CT_LOC_GIOU) g += dI * inv_c + k_c * (r.ch * dcw + r.cw * dch);
        else if (kind >= CT_LOC_DIOU) g -= k_c2 * (r.cw * dcw + r.ch * dch);
        return g;
    };
    const bool ox = r.iw > 0.f, oy = r.ih > 0.f;
    const float g_x1 = corner(ox && r.ax1 > r.tx1 ? -r.ih : 0.f, r.ax1 < r.tx1 ? -1.f : 0.f, 0.f);
    const float g_x2 = corner(ox && r.ax2 < r.tx2 ? r.ih : 0.f, r.ax2 > r.tx2 ? 1.f : 0.f, 0.f);
    const float g_y1 = corner(oy && r.ay1 > r.ty1 ? -r.iw : 0.f, 0.f, r.ay1 < r.ty1 ? -1.f : 0.f);
    const float g_y2 = corner(oy && r.ay2 < r.ty2 ? r.iw : 0.f, 0.f, r.ay2 > r.ty2 ? 1.f : 0.f);
    float g_w = r.iou * inv_u * r.ah, g_h = r.iou * inv_u * r.aw;
    float g_cx = 0.f, g_cy = 0.f;
    if (kind == CT_LOC_GIOU) {
        g_w -= r.ah * inv_c;
        g_h -= r.aw * inv_c;
    } else if (kind >= CT_LOC_DIOU) {
        g_cx = 2.f * (r.acx - r.tcx) / r.c2;
        g_cy = 2.f * (r.acy - r.tcy) / r.c2;
        if (kind == CT_LOC_CIOU) {
            const float dv = r.alpha * (2.f * IOU_FOUR_OVER_PI2) * r.dat / (r.aw * r.aw + r.ah * r.ah);
            g_w -= dv * r.ah;
            g_h += dv * r.aw;
        }
    }
    d0 = scale * (((g_x1 + g_x2) + g_cx) * (var0 * p.z));
    d1 = scale * (((g_y1 + g_y2) + g_cy) * (var0 * p.w));
    d2 = scale * (((g_x2 - g_x1) * 0.5f + g_w) * (r.aw * var1));
    d3 = scale * (((g_y2 - g_y1) * 0.5f + g_h) * (r.ah * var1));
}

}  // namespace ctdet
