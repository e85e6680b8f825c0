// Host-side launch code the direct convolution launchers share, written once (the style of ct_wino_launch.h: `who` first in
// every message, nothing here allocates):
//   conv_check_*       the descriptor checks ct_conv2d_fwd and ct_conv2d_x3_fwd have in common.  Three functions, not one:
//                      each launcher has checks of its own between them (packed-weight sizes, the f16x2 requirements, ...),
//                      and callers see the order in which a descriptor is judged;
//   conv_fill          what ConvArgs and X3Args have in common, for one batch chunk;
//   plan_splitk        the split-K plan of all three (ct_conv2d_bf16_fwd included).
// ct_conv2d_bf16_fwd has another contract (NHWC bf16, forward only, the whole batch under one descriptor) and keeps its checks.
#pragma once
#include "ct_common.h"
#include "ct_device.h"
#include "ct_f16x2.h"
#include <algorithm>

namespace ctdet {

// forward: (oh, ow) is the output size of an (h, w) input.  transposed (data gradient): (h, w) = spatial size of dY, (oh, ow) =
// spatial size of dX, the forward convolution's input.  Then the input channel slice.
inline int conv_check_sizes(const ct_conv_desc* d, const char* who)
{
    if (!d->transposed) {
        const int eoh = (d->h + 2 * d->pad_h - d->dil * (d->kh - 1) - 1) / d->stride + 1;
        const int eow = (d->w + 2 * d->pad_w - d->dil * (d->kw - 1) - 1) / d->stride + 1;
        CT_REQUIRE(eoh == d->oh && eow == d->ow, "%s: oh/ow %dx%d != expected %dx%d", who, d->oh, d->ow, eoh, eow);
    } else {
        const int fh = (d->oh + 2 * d->pad_h - d->dil * (d->kh - 1) - 1) / d->stride + 1;
        const int fw = (d->ow + 2 * d->pad_w - d->dil * (d->kw - 1) - 1) / d->stride + 1;
        CT_REQUIRE(fh == d->h && fw == d->w, "%s(transposed): dY %dx%d != forward output %dx%d of a %dx%d input", who, d->h, d->w,
                   fh, fw, d->oh, d->ow);
    }
    CT_REQUIRE(d->in_coff >= 0 && d->in_coff + d->cin <= d->in_ctot, "%s: input slice", who);
    return CT_OK;
}

// nseg, then the NCHW output and residual slices or the head segments
inline int conv_check_outputs(const ct_conv_desc* d, const char* who)
{
    CT_REQUIRE(d->nseg >= 0 && d->nseg <= 3, "%s: nseg", who);
    if (d->nseg == 0) {
        CT_REQUIRE(d->out && d->out_coff >= 0 && d->out_coff + d->cout <= d->out_ctot, "%s: output slice", who);
        CT_REQUIRE(!d->res || (d->res_coff >= 0 && d->res_coff + d->cout <= d->res_ctot), "%s: residual slice", who);
    } else {
        CT_REQUIRE(!d->res, "%s: residual with segmented output", who);
        for (int g = 0; g < d->nseg; ++g) CT_REQUIRE(d->seg[g].ptr, "%s: null segment", who);
    }
    return CT_OK;
}

// bytes of one input image (its buffer descriptor stays below 2 GiB) and how many images one launch may cover
inline int conv_check_image(const ct_conv_desc* d, const char* who, long long* img_in_bytes, int* max_chunk)
{
    *img_in_bytes = (long long)d->in_ctot * d->h * d->w * 4;
    CT_REQUIRE(*img_in_bytes < kMaxBufBytes, "%s: one image exceeds 2 GiB", who);
    *max_chunk = (int)std::max<long long>(1, kMaxBufBytes / *img_in_bytes);
    return CT_OK;
}

// What ConvArgs and X3Args share, for the images [b0, b0 + nb) of the batch.  The weights (pointer, bytes, M_pad), the k-step
// count, the tile counts and the split-K plan are the caller's.
template <typename Args>
inline void conv_fill(Args& a, const ct_conv_desc* d, int b0, int nb, long long img_in_bytes)
{
    a.OW = d->ow; a.OHW = d->oh * d->ow; a.Npix = nb * a.OHW;
    a.in = d->in + (size_t)b0 * d->in_ctot * d->h * d->w;
    a.scale = d->scale; a.shift = d->shift; a.lo = d->lo;
    a.res = d->res ? d->res + (size_t)b0 * d->res_ctot * a.OHW : nullptr;
    a.out = d->nseg == 0 ? d->out + (size_t)b0 * d->out_ctot * a.OHW : nullptr;
    a.nseg = d->nseg;
    for (int g = 0; g < d->nseg; ++g) {
        a.seg[g] = d->seg[g];
        a.seg[g].ptr += (size_t)b0 * d->seg[g].img_stride;
    }
    a.in_bytes = (unsigned)(img_in_bytes * nb);
    a.Cin = d->cin; a.H = d->h; a.W = d->w; a.in_ctot = d->in_ctot; a.in_coff = d->in_coff;
    a.M = d->cout;
    a.stride = d->stride; a.pad_h = d->pad_h; a.pad_w = d->pad_w; a.dil = d->dil;
    a.transposed = d->transposed;
    a.out_ctot = d->out_ctot; a.out_coff = d->out_coff;
    a.res_ctot = d->res_ctot; a.res_coff = d->res_coff; a.res_scale = d->res_scale;
    a.relu = d->relu;
    a.out_amax = d->out_absmax ? d->out_absmax + (size_t)b0 * h2::kLineWords : nullptr;      // one line per image
}

// Deterministic slab split-K: ksplit workgroups per tile, each over steps_per_split k-steps, partial sums in ws.
//   want          ct_conv_desc.ksplit: 0 / 1 none, > 1 that many (capped by the k-steps and the workspace), < 0 auto: aim at
//                 `target` workgroups (768 = ~3 per CU), at least two k-steps per split
//   slab_floats   cout x pixels of the launch: one split's partial sums
//   whole_batch   the launch covers the whole batch (the workspace is sized for it; a chunked launch does not split)
struct SplitK {
    int ksplit, steps_per_split;
};
inline SplitK plan_splitk(int want, int tiles, int nsteps, long long slab_floats, const float* ws, long long ws_floats,
                          bool whole_batch, int target)
{
    if (want < 0) want = tiles * 2 > target ? 1 : std::min(nsteps / 2, target / tiles);
    if (ws && slab_floats > 0) want = (int)std::min<long long>(want, ws_floats / slab_floats);
    if (!(want > 1 && ws && whole_batch && nsteps >= 2 && slab_floats < 0x7FFFFFFFLL)) return {1, nsteps};
    const int steps_per_split = (nsteps + std::min(want, nsteps) - 1) / std::min(want, nsteps);
    return {(nsteps + steps_per_split - 1) / steps_per_split, steps_per_split};
}

}  // namespace ctdet
