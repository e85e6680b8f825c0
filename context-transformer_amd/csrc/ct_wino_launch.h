// Host-side launch prologue of the five Winograd forward launchers (ct_wino, ct_wino4, ct_wino_x3, ct_wino4f, ct_wino4s),
// written once: the argument checks in the order callers see them, the per-image byte counts with the batch chunking that keeps
// every buffer descriptor below 2 GiB, and the fill of what the launchers' kernel-argument records have in common.  Nothing here
// allocates.  Checks that belong to one launcher (variant, workspace, packed-weight size, ...) stay in that launcher.
#pragma once
#include "ct_common.h"
#include "ct_device.h"
#include <algorithm>

namespace ctdet {

// the optional fused 2x2 / stride 2 max-pool output of a launch (pool_out null: none) and whether the full map is stored too
struct PoolOut {
    float* pool_out;
    int pool_ctot, pool_coff, pool_oh, pool_ow, write_full;
};

// bytes of one image of each tensor, and how many images one launch may cover
struct WinoLimits {
    long long img_in_bytes, img_out_bytes, img_res_bytes;
    int max_chunk;
};

// Pointers and geometry.  supported = d && the launcher's own geometry predicate; needs = that geometry in words.
inline int wino_check_desc(const ct_conv_desc* d, bool pointers, bool supported, const char* who, const char* needs)
{
    CT_REQUIRE(d && pointers, "%s: null pointer", who);
    CT_REQUIRE(d->in && (d->out || d->nseg > 0) && d->scale && d->shift, "%s: null tensor", who);
    if (!supported)
        return fail(CT_ERR_UNSUPPORTED, "%s: needs %s (got %dx%d s%d d%d p%d cin=%d nseg=%d)", who, needs, d->kh, d->kw,
                    d->stride, d->dil, d->pad_h, d->cin, d->nseg);
    return CT_OK;
}

// Shape, pooled output, input / output / residual slices, segments, the 2 GiB limit per image; fills lim.
inline int wino_check_launch(const ct_conv_desc* d, const char* who, const PoolOut& p, WinoLimits* lim)
{
    CT_REQUIRE(d->batch > 0 && d->cout > 0, "%s: bad shape", who);
    CT_REQUIRE(p.write_full || p.pool_out, "%s: nothing to write", who);
    if (p.pool_out) {
        CT_REQUIRE(p.pool_coff >= 0 && p.pool_coff + d->cout <= p.pool_ctot, "%s: pooled output slice", who);
        CT_REQUIRE((p.pool_oh == d->oh / 2 || p.pool_oh == (d->oh + 1) / 2) && (p.pool_ow == d->ow / 2 || p.pool_ow == (d->ow + 1) / 2),
                   "%s: pooled size %dx%d for a %dx%d map", who, p.pool_oh, p.pool_ow, d->oh, d->ow);
    }
    CT_REQUIRE(d->in_coff >= 0 && d->in_coff + d->cin <= d->in_ctot, "%s: input slice", who);
    if (d->nseg == 0)
        CT_REQUIRE(d->out_coff >= 0 && d->out_coff + d->cout <= d->out_ctot, "%s: output slice", who);
    else {
        CT_REQUIRE(!p.pool_out && p.write_full, "%s: pooling with segmented output", who);
        for (int g = 0; g < d->nseg; ++g) CT_REQUIRE(d->seg[g].ptr, "%s: null segment", who);
    }
    CT_REQUIRE(!d->res || (d->res_coff >= 0 && d->res_coff + d->cout <= d->res_ctot), "%s: residual slice", who);
    lim->img_in_bytes = (long long)d->in_ctot * d->h * d->w * 4;
    CT_REQUIRE(lim->img_in_bytes < kMaxBufBytes, "%s: one image exceeds 2 GiB", who);
    lim->img_out_bytes = d->nseg ? 4 : (long long)d->out_ctot * d->oh * d->ow * 4;
    lim->img_res_bytes = d->res ? (long long)d->res_ctot * d->oh * d->ow * 4 : 0;
    CT_REQUIRE(lim->img_out_bytes < kMaxBufBytes && lim->img_res_bytes < kMaxBufBytes, "%s: one image exceeds 2 GiB", who);
    lim->max_chunk = (int)std::max<long long>(1, kMaxBufBytes / std::max(lim->img_in_bytes, std::max(lim->img_out_bytes, lim->img_res_bytes)));
    return CT_OK;
}

// What the five argument records share, for the images [b0, b0 + nb) of the batch.  Args is WinoArgs, Wino4Args, WinoX3Args,
// Wino4fArgs or Wino4sArgs: kernel-argument layouts of their own that agree in these member names (as ct_wino4_emit.h relies on).
// tile = 2 or 4: output tile edge of a dilation-1 form, sets TY / TX / NT; 0 leaves them to the caller (wino4s: sizes_of).
template <typename Args>
inline void wino_fill(Args& a, const ct_conv_desc* d, const void* upacked, const WinoLimits& lim, const PoolOut& p, int b0, int nb,
                      int tile)
{
    const int OHW = d->oh * d->ow;
    a.in = d->in + (size_t)b0 * d->in_ctot * d->h * d->w;
    a.U = static_cast<decltype(a.U)>(upacked);
    a.scale = d->scale; a.shift = d->shift; a.lo = d->lo;
    a.res = d->res ? d->res + (size_t)b0 * d->res_ctot * OHW : nullptr;
    a.out = d->nseg ? nullptr : d->out + (size_t)b0 * d->out_ctot * OHW;
    a.nseg = d->nseg;
    for (int g = 0; g < d->nseg; ++g) {
        a.seg[g] = d->seg[g];
        a.seg[g].ptr += (size_t)b0 * d->seg[g].img_stride;
    }
    a.in_bytes = (unsigned)(lim.img_in_bytes * nb);
    a.out_bytes = (unsigned)(lim.img_out_bytes * nb);
    a.res_bytes = (unsigned)(lim.img_res_bytes * nb);
    a.Cin = d->cin; a.H = d->h; a.W = d->w; a.in_ctot = d->in_ctot; a.in_coff = d->in_coff;
    a.M = d->cout;
    if (tile) {
        a.TY = (d->oh + tile - 1) / tile; a.TX = (d->ow + tile - 1) / tile;
        a.NT = nb * a.TY * a.TX;
    }
    a.out_ctot = d->out_ctot; a.out_coff = d->out_coff;
    a.res_ctot = d->res_ctot; a.res_coff = d->res_coff; a.res_scale = d->res_scale;
    a.relu = d->relu;
    a.pool_out = p.pool_out ? p.pool_out + (size_t)b0 * p.pool_ctot * p.pool_oh * p.pool_ow : nullptr;
    a.pool_ctot = p.pool_ctot; a.pool_coff = p.pool_coff; a.pool_oh = p.pool_oh; a.pool_ow = p.pool_ow;
    a.write_full = p.write_full;
}

}  // namespace ctdet
