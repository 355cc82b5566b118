// Control zones (solvers.ControlZones; an extension, no reference call): controls that are piecewise constant in space on
// m sets of nodes.  With chi_j the nodal indicator of zone j (the P1 function that is 1 on the zone's nodes) the
// directions live in span{chi_j} per time level, and
//   femfct_set_control_zones   validates the labels and builds the device table
//   femfct_zone_restrict       out[f][j] = sum_{i in zone j} y_i, y = x_f or M x_f: chi^T x / chi^T M x, `fields` fields a call
//   femfct_zone_prolong        out[f][i] = (Ginv s_f)[label_i], 0.0 at an unlabelled node
// With G = chi^T M chi (m x m, SPD) prolong(Ginv . restrict(M x)) is the orthogonal projection in the mass inner product,
// and prolong(Ginv . restrict(r)) the steepest-descent direction among zone-constant controls for a dual vector r: an
// m x m product per level where the free control needs a mass solve.
//
// k_zone_restrict is a gather sum: a zone's node list (ascending) is cut into chunks of ZN_CH nodes, one block each; lane t
// reads list entries t, t + blockDim, .. (unit stride) and gathers x there -- with the mass matrix the row k_quadform
// forms, diagonal slot first, then slots 1..W-1 -- adds its up to ZN_PT values in that order in a register, and the block
// folds the lanes' sums in block_reduce's tree.  Where a zone has more than one chunk k_zone_restrict_fold adds the chunk
// sums in order from a partials buffer.  A table whose largest zone fits one wave's ZN_PT entries per lane (256 nodes)
// runs one wave per block (no LDS, no barrier: many small zones are many small blocks), as k_time_restrict does for short
// intervals.  The order of a zone's sum is fixed by the table alone: no atomics, the same bits for every number of
// fields, every position of a field and every run.  The pointwise expressions have no contraction
// (-ffp-contract=off).
#include "femfct_internal.h"
#include "device_utils.h"

#include <vector>

#define ZN_BLOCK 256
#define ZN_PT 4                                    // list entries per thread
#define ZN_CH (ZN_BLOCK * ZN_PT)                   // nodes per chunk

namespace {

// Device table (int32): off[m+1] (zone j = list entries off[j] <= q < off[j+1]), first work item of zone j [m+1], first
// partial of zone j [m+1] (a zone of one chunk has none), zone of work item [items], list [listed], label [n].
struct ZoneTable { const int32_t *off, *ifirst, *pfirst, *item_zone, *list, *label; int m, items, nparts; };

ZoneTable zone_table(const femfct_ctx* ctx) {
    const int32_t* d = ctx->d_ztab;
    const int m = ctx->zn_m;
    return ZoneTable{d, d + (m + 1), d + 2 * (m + 1), d + 3 * (m + 1), d + 3 * (m + 1) + ctx->zn_items,
                     d + 3 * (m + 1) + ctx->zn_items + ctx->zn_listed, m, ctx->zn_items, ctx->zn_nparts};
}

// block = chunk blockIdx.x of the table; the fields are strided over gridDim.y.  blockDim.x = ZN_BLOCK, or WAVE when no
// zone is longer than WAVE * ZN_PT.
template <bool MASS>
__global__ void __launch_bounds__(ZN_BLOCK) k_zone_restrict(int n, int W, const int32_t* __restrict__ cols,
                                                            const double* __restrict__ M, ZoneTable t, int64_t fields,
                                                            const double* __restrict__ x, double* __restrict__ out,
                                                            double* __restrict__ part) {
    __shared__ double smem[32];
    const int it = blockIdx.x, j = t.item_zone[it], c = it - t.ifirst[j];
    const int s = t.off[j], e = t.off[j + 1];
    const int c0 = s + c * ZN_CH, c1 = min(c0 + ZN_CH, e);           // this block's chunk of the list
    int node[ZN_PT];
#pragma unroll
    for (int q = 0; q < ZN_PT; ++q) {
        const int l = c0 + q * (int)blockDim.x + (int)threadIdx.x;
        node[q] = l < c1 ? t.list[l] : -1;
    }
    for (int64_t f = blockIdx.y; f < fields; f += gridDim.y) {
        const double* xf = x + f * n;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < ZN_PT; ++q) {
            const int i = node[q];
            if (i < 0) continue;
            double y;
            if (MASS) {
                y = M[i] * xf[i];
                for (int k = 1; k < W; ++k) {
                    const int64_t idx = (int64_t)k * n + i;
                    y += M[idx] * xf[cols[idx]];
                }
            } else {
                y = xf[i];
            }
            acc += y;
        }
        acc = block_reduce(acc, OpSum(), 0.0, smem);
        if (threadIdx.x == 0) {
            if (e - s <= ZN_CH) out[f * t.m + j] = acc;
            else part[f * t.nparts + t.pfirst[j] + c] = acc;
        }
    }
}

// the zones of more than one chunk: out = the chunk sums added in order; one thread per (field, zone)
__global__ void k_zone_restrict_fold(ZoneTable t, int64_t fields, const double* __restrict__ part, double* __restrict__ out) {
    const int64_t work = fields * t.m;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < work; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = q / t.m;
        const int j = (int)(q % t.m), len = t.off[j + 1] - t.off[j];
        if (len <= ZN_CH) continue;
        const int nch = (len + ZN_CH - 1) / ZN_CH;
        const double* p = part + f * t.nparts + t.pfirst[j];
        double acc = p[0];
        for (int c = 1; c < nch; ++c) acc += p[c];
        out[q] = acc;
    }
}

// delta[f][j] = ((Ginv[j][0] s[f][0] + Ginv[j][1] s[f][1]) + ..): once per field, one thread per (field, zone)
__global__ void k_zone_coeff(int m, int64_t fields, const double* __restrict__ Ginv, const double* __restrict__ s,
                             double* __restrict__ delta) {
    const int64_t work = fields * m;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < work; q += (int64_t)gridDim.x * blockDim.x) {
        const double* sf = s + (q / m) * m;
        const double* g = Ginv + (int64_t)(q % m) * m;
        double acc = g[0] * sf[0];
        for (int k = 1; k < m; ++k) acc += g[k] * sf[k];
        delta[q] = acc;
    }
}

// out[f][i] = delta[f][label_i], 0.0 at an unlabelled node; the fields are strided over gridDim.y
__global__ void k_zone_scatter(int n, ZoneTable t, int64_t fields, const double* __restrict__ delta, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = t.label[i];
    for (int64_t f = blockIdx.y; f < fields; f += gridDim.y) out[f * n + i] = j >= 0 ? delta[f * t.m + j] : 0.0;
}

unsigned grid_y(int64_t work) { return (unsigned)(work < 65535 ? work : 65535); }

unsigned flat_grid(int64_t work) {
    int64_t g = (work + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 65535 ? 65535 : g);
}

}  // namespace

extern "C" {

int femfct_set_control_zones(femfct_ctx* ctx, const int32_t* labels_host, int32_t m) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0, "pattern not set");
    if (!labels_host) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (launches that read the table may be in flight)
        if (ctx->d_ztab) hipFree(ctx->d_ztab);
        ctx->d_ztab = nullptr;
        ctx->zn_m = ctx->zn_items = ctx->zn_nparts = ctx->zn_listed = ctx->zn_maxlen = 0;
        return FEMFCT_OK;
    }
    ARG_TRY(ctx, m >= 1 && m <= FEMFCT_MAX_ZONES, "m (zones) must be in 1..256");
    const int n = ctx->n;
    std::vector<int32_t> size((size_t)m, 0);
    for (int i = 0; i < n; ++i) {
        ARG_TRY(ctx, labels_host[i] >= -1 && labels_host[i] < m, "labels must lie in -1 .. m-1");
        if (labels_host[i] >= 0) ++size[labels_host[i]];
    }
    std::vector<int32_t> off((size_t)m + 1), ifirst((size_t)m + 1), pfirst((size_t)m + 1), item_zone;
    int items = 0, nparts = 0, listed = 0, maxlen = 0;
    for (int j = 0; j < m; ++j) {
        ARG_TRY(ctx, size[j] > 0, "every zone must hold at least one node");
        const int nch = (size[j] + ZN_CH - 1) / ZN_CH;
        off[j] = listed;
        ifirst[j] = items;
        pfirst[j] = nparts;
        listed += size[j];
        items += nch;
        if (nch > 1) nparts += nch;
        if (size[j] > maxlen) maxlen = size[j];
        item_zone.insert(item_zone.end(), (size_t)nch, j);
    }
    off[m] = listed;
    ifirst[m] = items;
    pfirst[m] = nparts;
    std::vector<int32_t> list((size_t)listed), fill(off.begin(), off.end() - 1);
    for (int i = 0; i < n; ++i)                                   // ascending within every zone
        if (labels_host[i] >= 0) list[(size_t)fill[labels_host[i]]++] = i;
    std::vector<int32_t> h(off);
    h.insert(h.end(), ifirst.begin(), ifirst.end());
    h.insert(h.end(), pfirst.begin(), pfirst.end());
    h.insert(h.end(), item_zone.begin(), item_zone.end());
    h.insert(h.end(), list.begin(), list.end());
    h.insert(h.end(), labels_host, labels_host + n);
    int32_t* d = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d, sizeof(int32_t) * h.size()));
    hipError_t e = hipMemcpyAsync(d, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // h is read, and no launch reads the old table any more
    if (e != hipSuccess) {
        hipFree(d);
        return femfct_fail(ctx, FEMFCT_ERR_HIP, "zone table upload failed: %s", hipGetErrorString(e));
    }
    if (ctx->d_ztab) hipFree(ctx->d_ztab);
    ctx->d_ztab = d;
    ctx->zn_m = m;
    ctx->zn_items = items;
    ctx->zn_nparts = nparts;
    ctx->zn_listed = listed;
    ctx->zn_maxlen = maxlen;
    return FEMFCT_OK;
}

int femfct_zone_restrict(femfct_ctx* ctx, const double* x_dev, int64_t fields, int32_t apply_mass, double* out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->zn_m > 0 && ctx->d_ztab, "control zones not set");
    ARG_TRY(ctx, x_dev && out_dev && fields >= 1, "bad argument");
    ARG_TRY(ctx, apply_mass == 0 || apply_mass == 1, "apply_mass must be 0 or 1");
    ARG_TRY(ctx, !apply_mass || ctx->have_mass, "mass matrix not set");
    const ZoneTable t = zone_table(ctx);
    if (t.nparts) {
        int rc = femfct_ensure_scratch(ctx, (size_t)fields * t.nparts);
        if (rc != FEMFCT_OK) return rc;
    }
    const dim3 grid((unsigned)t.items, grid_y(fields)), block(ctx->zn_maxlen <= WAVE * ZN_PT ? WAVE : ZN_BLOCK);
    if (apply_mass)
        hipLaunchKernelGGL(k_zone_restrict<true>, grid, block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M, t,
                           fields, x_dev, out_dev, ctx->d_scratch);
    else
        hipLaunchKernelGGL(k_zone_restrict<false>, grid, block, 0, ctx->stream, ctx->n, ctx->W, ctx->d_cols, ctx->d_M,
                           t, fields, x_dev, out_dev, ctx->d_scratch);
    if (t.nparts)
        hipLaunchKernelGGL(k_zone_restrict_fold, dim3(flat_grid(fields * t.m)), dim3(256), 0, ctx->stream, t, fields,
                           ctx->d_scratch, out_dev);
    return FEMFCT_OK;
}

int femfct_zone_prolong(femfct_ctx* ctx, const double* s_dev, const double* Ginv_dev, int64_t fields, double* out_dev) {
    FEMFCT_ENTER(ctx);
    ARG_TRY(ctx, ctx->n > 0 && ctx->zn_m > 0 && ctx->d_ztab, "control zones not set");
    ARG_TRY(ctx, s_dev && out_dev && fields >= 1, "bad argument");
    const ZoneTable t = zone_table(ctx);
    const double* delta = s_dev;
    if (Ginv_dev) {
        int rc = femfct_ensure_scratch(ctx, (size_t)fields * t.m);
        if (rc != FEMFCT_OK) return rc;
        hipLaunchKernelGGL(k_zone_coeff, dim3(flat_grid(fields * t.m)), dim3(256), 0, ctx->stream, t.m, fields, Ginv_dev, s_dev,
                           ctx->d_scratch);
        delta = ctx->d_scratch;
    }
    hipLaunchKernelGGL(k_zone_scatter, dim3((unsigned)((ctx->n + 255) / 256), grid_y(fields)), dim3(256), 0, ctx->stream,
                       ctx->n, t, fields, delta, out_dev);
    return FEMFCT_OK;
}

}  // extern "C"
