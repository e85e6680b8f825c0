// Host-side launch code the five weight-gradient launchers share (ct_conv2d_wgrad, _wino, _wino4, _wino4s, _h2), written once in the
// style of ct_wino_launch.h (`who` first in every message, nothing here allocates): the pointer and slice checks, the byte counts
// with the 2 GiB limit and the batch chunking, the fill of what the kernel-argument records share, the rounding of a split plan, and
// the whole launcher of the two fused Winograd kernels, which differ in numbers only.  Each launcher calls these in the order it
// judges a descriptor, with its own checks between them (geometry predicate, oh/ow, workspace size, ...); how many splits it WANTS
// is its own tuning and stays with it.
#pragma once
#include "ct_common.h"
#include "ct_device.h"
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace ctdet {

// names the pointer that is null; no_workspace(): the `workspace` of a launcher that takes none
inline const void* no_workspace() { static const char here = 0; return &here; }
inline int wgrad_check_pointers(const ct_conv_desc* d, const float* dz, const float* dw, const void* workspace, const char* who)
{
    CT_REQUIRE(d, "%s: d is null", who);
    CT_REQUIRE(d->in, "%s: d->in is null", who);
    CT_REQUIRE(dz, "%s: dz is null", who);
    CT_REQUIRE(dw, "%s: dw is null", who);
    CT_REQUIRE(workspace, "%s: workspace is null", who);
    return CT_OK;
}

inline int wgrad_check_slices(const ct_conv_desc* d, int dz_ctot, int dz_coff, const char* who)
{
    CT_REQUIRE(d->batch > 0 && d->cin > 0 && d->cout > 0, "%s: bad shape", who);
    CT_REQUIRE(d->in_coff >= 0 && d->in_coff + d->cin <= d->in_ctot, "%s: input slice", who);
    CT_REQUIRE(dz_coff >= 0 && dz_coff + d->cout <= dz_ctot, "%s: dz slice", who);
    return CT_OK;
}

// bytes of one image and of the whole batch of X and dZ (32-bit buffer offsets: a descriptor stays below 2 GiB), and how many
// images one launch may cover
struct WgradLimits { long long img_x_bytes, img_z_bytes, x_bytes, z_bytes; int max_chunk; };

inline WgradLimits wgrad_sizes(const ct_conv_desc* d, int dz_ctot, long long launch_max = kMaxBufBytes)
{
    WgradLimits l{};
    l.img_x_bytes = (long long)d->in_ctot * d->h * d->w * 4;
    l.img_z_bytes = (long long)dz_ctot * d->oh * d->ow * 4;
    l.x_bytes = l.img_x_bytes * d->batch;
    l.z_bytes = l.img_z_bytes * d->batch;
    l.max_chunk = (int)std::max<long long>(1, launch_max / std::max<long long>(1, std::max(l.img_x_bytes, l.img_z_bytes)));
    return l;
}

// launch_max: the bytes of either tensor one launch may cover (ct_conv2d_wgrad stays one byte below the others)
inline int wgrad_limits(const ct_conv_desc* d, int dz_ctot, const char* who, WgradLimits* lim, long long launch_max = kMaxBufBytes)
{
    *lim = wgrad_sizes(d, dz_ctot, launch_max);
    CT_REQUIRE(lim->img_x_bytes < kMaxBufBytes && lim->img_z_bytes < kMaxBufBytes, "%s: one image exceeds 2 GiB", who);
    return CT_OK;
}

// The members the four argument records share, for the images [b0, b0 + nb) of the batch.  Kernel-argument layouts of their own
// that agree in these names; everything else (geometry, tiles, splits, outputs) is the caller's.
template <typename Args>
inline void wgrad_fill(Args& a, const ct_conv_desc* d, const float* dz, int dz_ctot, int dz_coff, const WgradLimits& lim, int b0, int nb)
{
    a.x = d->in + (size_t)b0 * (lim.img_x_bytes / 4);
    a.dz = dz + (size_t)b0 * (lim.img_z_bytes / 4);
    a.x_bytes = (unsigned)(lim.img_x_bytes * nb);
    a.dz_bytes = (unsigned)(lim.img_z_bytes * nb);
    a.Cin = d->cin; a.Cout = d->cout;
    a.x_ctot = d->in_ctot; a.x_coff = d->in_coff; a.dz_ctot = dz_ctot; a.dz_coff = dz_coff;
}

// `units` of work over about `want` splits: the share of a split rounded up, and the splits that are then not empty
struct Split { int splits, per_split; };
inline Split even_split(int units, int want)
{
    const int per_split = (units + want - 1) / want;
    return {(units + per_split - 1) / per_split, per_split};
}

// The slab workspace of a deterministic (_det) entry: every split stores its partial result in a slab of its own and a finishing
// kernel adds the slabs in slab-index order.  The producers write every element of every slab the finish reads, so the workspace
// may hold anything on entry and ct_scratch_prezeroed has no bearing on it.
inline int wgrad_check_det_workspace(const void* workspace, size_t have, size_t need, const char* who)
{
    CT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    if (have < need) return fail(CT_ERR_WORKSPACE, "%s: workspace_bytes %zu, needs %zu", who, have, need);
    return CT_OK;
}

// out[i] = slab 0 [i] + slab 1 [i] + ... of `nslabs` slabs of n floats, in slab-index order: one thread per element, so the order
// is the loop's (the loads of four slabs are issued together, the additions stay in order).  out may be slab 0 itself.
__global__ static __launch_bounds__(256) void wgrad_slab_sum_kernel(const float* slabs, int nslabs, size_t n, float* out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = slabs[i];
#pragma unroll 4
    for (int s = 1; s < nslabs; ++s) v += slabs[(size_t)s * n + i];
    out[i] = v;
}

inline int wgrad_slab_sum(const float* slabs, int nslabs, size_t n, float* out, hipStream_t st)
{
    hipLaunchKernelGGL(wgrad_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slabs, nslabs, n, out);
    CT_LAUNCH_CHECK("wgrad_slab_sum_kernel");
    return CT_OK;
}

// ---- the two fused Winograd kernels: F(3x3, 2x2) of ct_wino_wgrad.hip and F(3x3, 4x4) of ct_wino4_wgrad.hip
inline bool wgrad_wino_ok(const ct_conv_desc* d)
{
    return d->kh == 3 && d->kw == 3 && d->stride == 1 && d->dil == 1 && d->pad_h == 1 && d->pad_w == 1 &&
           d->oh == d->h && d->ow == d->w && !d->transposed && d->cin >= 1 && d->cout >= 1 &&
           (long long)d->in_ctot * d->h * d->w * 4 < kMaxBufBytes;
}

struct WinoWgradForm {
    const char *who, *kernel_name, *finish_name;
    int tile, points;           // output tile edge, transform points = (tile + 2)^2
    int block, threads;         // channels per workgroup side, threads per workgroup
    int lds_bytes;
    int (*wgs)();               // workgroups to aim at (one round of the chip, or what the form's environment variable says): read
                                // once per kernel and process, by the form's own function
    bool det;                   // the _det entry: one dU slab per split, summed in order ahead of `finish`, in place of the atomics
};

// The tile-range splits of a launch over nb images: a pure function of the descriptor and the environment (host only).
struct WinoWgradPlan { int TY, TX, NT, chunks, cblocks, blocks; Split sp; };
inline WinoWgradPlan wgrad_wino_plan(const WinoWgradForm& f, const ct_conv_desc* d, int nb)
{
    WinoWgradPlan p{};
    const int kblocks = (d->cout + f.block - 1) / f.block;
    p.cblocks = (d->cin + f.block - 1) / f.block;
    p.blocks = kblocks * p.cblocks;
    const int wgs = f.wgs();
    p.TY = (d->h + f.tile - 1) / f.tile; p.TX = (d->w + f.tile - 1) / f.tile;
    p.NT = nb * p.TY * p.TX;
    p.chunks = (p.NT + 7) / 8;                     // TT = 8 tiles per chunk in both kernels
    p.sp = even_split(p.chunks, std::min(65535, std::max(1, std::min(p.chunks, wgs / p.blocks))));
    return p;
}

// splits of all batch chunks of a launch, in chunk order: the dU slabs of a _det entry
inline int wgrad_wino_total_splits(const WinoWgradForm& f, const ct_conv_desc* d, const WgradLimits& lim)
{
    int total = 0;
    for (int b0 = 0; b0 < d->batch; b0 += lim.max_chunk) total += wgrad_wino_plan(f, d, std::min(lim.max_chunk, d->batch - b0)).sp.splits;
    return total;
}

// bytes of the slab workspace of a _det entry (dZ taken as dense), 0 for a descriptor the form does not take; *partials = slabs
inline size_t wgrad_wino_det_bytes(const WinoWgradForm& f, const ct_conv_desc* d, int* partials)
{
    if (partials) *partials = 0;
    if (!d || !wgrad_wino_ok(d) || d->batch <= 0) return 0;
    const WgradLimits lim = wgrad_sizes(d, d->cout);
    if (lim.img_x_bytes >= kMaxBufBytes || lim.img_z_bytes >= kMaxBufBytes) return 0;
    const int total = wgrad_wino_total_splits(f, d, lim);
    if (partials) *partials = total;
    return (size_t)total * f.points * d->cout * d->cin * sizeof(float);
}

// Workgroup = block x block channels x all transform points over a range of tile chunks; the ranges are split over
// blockIdx.y, partial sums meet in the workspace dU[points][cout][cin] through f32 atomics, `finish` applies G^T . G into dw.
// f.det: split s of the launch stores slab s of dU[splits][points][cout][cin] (workspace_bytes of them; nothing is zeroed),
// wgrad_slab_sum adds the slabs in order into slab 0, and `finish` runs on that.
template <typename Args>
int launch_wgrad_wino(const WinoWgradForm& f, void (*kernel)(Args), void (*finish)(const float*, float*, int), const ct_conv_desc* d,
                      const float* dz, int dz_ctot, int dz_coff, float* dw, void* workspace, size_t workspace_bytes, ct_stream_t stream)
{
    if (int rc = wgrad_check_pointers(d, dz, dw, workspace, f.who)) return rc;
    if (!wgrad_wino_ok(d))
        return fail(CT_ERR_UNSUPPORTED, "%s: needs 3x3 stride 1 dilation 1 pad 1 (got %dx%d s%d d%d p%d)", f.who, d->kh, d->kw,
                    d->stride, d->dil, d->pad_h);
    if (int rc = wgrad_check_slices(d, dz_ctot, dz_coff, f.who)) return rc;
    WgradLimits lim;
    if (int rc = wgrad_limits(d, dz_ctot, f.who, &lim)) return rc;
    const int KC = d->cout * d->cin;
    const size_t slab = (size_t)f.points * KC;          // floats
    if (f.det)
        if (int rc = wgrad_check_det_workspace(workspace, workspace_bytes, wgrad_wino_total_splits(f, d, lim) * slab * sizeof(float), f.who))
            return rc;
    hipStream_t st = as_stream(stream);
    CT_HIP(raise_lds_limit((const void*)kernel, f.lds_bytes));
    float* dU = static_cast<float*>(workspace);
    if (!f.det && !scratch_prezeroed()) CT_HIP(hipMemsetAsync(dU, 0, slab * 4, st));
    int slabs = 0;
    for (int b0 = 0; b0 < d->batch; b0 += lim.max_chunk) {
        const int nb = std::min(lim.max_chunk, d->batch - b0);
        const WinoWgradPlan p = wgrad_wino_plan(f, d, nb);
        Args a{};
        wgrad_fill(a, d, dz, dz_ctot, dz_coff, lim, b0, nb);
        a.dU = dU;
        a.slab = f.det ? dU + slabs * slab : nullptr;
        a.H = d->h; a.W = d->w;
        a.TY = p.TY; a.TX = p.TX;
        a.NT = p.NT;
        a.chunks = p.chunks;
        a.cblocks = p.cblocks;
        a.chunks_per_split = p.sp.per_split;
        hipLaunchKernelGGL(kernel, dim3(p.blocks, p.sp.splits), dim3(f.threads), f.lds_bytes, st, a);
        CT_LAUNCH_CHECK(f.kernel_name);
        slabs += p.sp.splits;
    }
    if (f.det && slabs > 1)
        if (int rc = wgrad_slab_sum(dU, slabs, slab, dU, st)) return rc;
    hipLaunchKernelGGL(finish, dim3((KC + 255) / 256), dim3(256), 0, st, dU, dw, KC);
    CT_LAUNCH_CHECK(f.finish_name);
    return CT_OK;
}

}  // namespace ctdet
