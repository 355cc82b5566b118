// 32 x 32 tile kernels of the structured mesh in vertex order -- the LATENCY regime (the config meshes, n = 1681 / 6561:
// a sweep moves < 1 MB and costs one dependent kernel boundary, so the step is bound by its number of launches).
// Selected by femfct_tile_plan (policy block at the end of this file, with femfct_tile_big and
// femfct_cheb_flux_fusable); larger meshes and batches go to kernels_patch64.hip, other patterns to kernels_rowstrip.hip.
// A step of this regime, launch by launch: k_tile_build_jacobi (operator + first sweeps; k_low_seq builds the operators
// of a whole sequence beforehand), k_tile_jacobi, k_tile_dudt_cheb, k_tile_cheb, then k_tile_cheb_flux_limit or
// k_tile_flux_limit.
//
// A 1024-thread workgroup stages a 32 x 32 patch = (32 - 2H)^2 tile + halo H on every side -- one node per thread, the
// node's matrix row in registers, the iterate in LDS -- and runs up to H sweeps per launch (the halo shrinks by one
// ring per sweep).  H = 8 on large grids (least re-reading), 8..13 in the latency regime (fewest launches: see
// femfct_tile_plan).  Compared with row strips there is no column table to load and the work spreads over
// (N / (32 - 2H))^2 workgroups.  The two fused launches behind the Jacobi solve also run on fitted patches of 26 and 30
// nodes per side (6 x 6 tiles, FEMFCT_TILE_FIT: femfct_tile_fit) while every workgroup gets a compute unit of its own.
#include "femfct_internal.h"
#include "device_utils.h"
#include "solve_ctl.h"
#include "forms.h"
#include "step_end.h"
#include "sweep_common.h"

#include <math.h>

#define TILE_T 16
#define TILE_H 8
#define TILE_L 32
#define TILE_LD 33   // padded LDS row
#define TILE_HMAX 13 // deepest halo instantiated (Jacobi, latency regime)

namespace {

// Phase stamps of the four launches of a latency-regime step (make tuning; FEMFCT_TILE_TRACE=<file>): the first lane of
// the wave that holds the tile's first owned node (it works through the kernel's last instruction whatever the epilogue
// does), in a workgroup in the middle of the grid, reads the 100 MHz clock at entry, once every load of the load phase
// is back (behind the barrier that publishes the staged iterate), behind the barrier of the last sweep or iteration (in
// the limiter also behind the barrier between fluxes and limiter) and at the end, and adds the differences to sums
// that femfct_tile_phase_dump writes out.  Read the shares, not the lengths.  The product library carries none of it.
#ifdef FEMFCT_TUNING
__device__ unsigned long long g_tile_phase[4][6];        // [kernel][ticks: load phase, in all, launches, to the last sweep's barrier, to the flux barrier, unused]
#define TILE_STAMP_BEGIN(thread)                                                                                        \
    unsigned long long ts0_ = 0, ts1_ = 0, ts3_ = 0, ts4_ = 0;                                                          \
    const bool ts_on_ = (int)threadIdx.x == (thread) / WAVE * WAVE && blockIdx.z == 0 && blockIdx.x == gridDim.x / 2 && blockIdx.y == gridDim.x / 2; \
    if (ts_on_) ts0_ = ts3_ = ts4_ = __builtin_amdgcn_s_memrealtime()
#define TILE_STAMP_LOADED() do { if (ts_on_) { __builtin_amdgcn_s_waitcnt(0); ts1_ = __builtin_amdgcn_s_memrealtime(); } } while (0)
#define TILE_STAMP_SWEPT() do { if (ts_on_) ts3_ = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TILE_STAMP_FLUXES() do { if (ts_on_) ts4_ = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TILE_STAMP_END(id) do { if (ts_on_) {                                                                           \
        const unsigned long long ts2_ = __builtin_amdgcn_s_memrealtime();                                               \
        g_tile_phase[id][0] += ts1_ - ts0_; g_tile_phase[id][1] += ts2_ - ts0_; g_tile_phase[id][2] += 1;               \
        g_tile_phase[id][3] += ts3_ - ts0_; g_tile_phase[id][4] += ts4_ - ts0_; } } while (0)
#else
#define TILE_STAMP_BEGIN(thread) do { } while (0)
#define TILE_STAMP_LOADED() do { } while (0)
#define TILE_STAMP_SWEPT() do { } while (0)
#define TILE_STAMP_FLUXES() do { } while (0)
#define TILE_STAMP_END(id) do { } while (0)
#endif

// The output stores of the four launches.  TILE_TRIM_WT (FEMFCT_TILE_TRIM bit 8): agent-scope relaxed atomic stores, which
// are plain write-through stores (sc1) -- no dirty line is left for the write-back at the kernel's end.  The value stored
// is the same; whoever reads it is a later launch.
#define TILE_OUT(lvalue, value) do {                                                                                    \
        if constexpr ((TRIM & 8) != 0) __hip_atomic_store(&(lvalue), (value), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
        else (lvalue) = (value); } while (0)

struct TileGeom {
    int lx, ly, gx, gy, i;
    bool inside, owned;      // (both false for the spare threads of a patch that is no whole number of waves)
    int kvalid;          // the node's value is exact for sweeps k < kvalid
    int nb[6];           // LDS offsets of the six neighbours (clamped into the patch)
    int self;
};

template <int T = TILE_T, int H = TILE_H, int PL = TILE_L>
__device__ __forceinline__ TileGeom tile_geom(int N) {
    static_assert(T + 2 * H == PL, "patch edge = tile + 2 halos");
    constexpr int PLD = PL + 1;
    TileGeom g;
    g.lx = threadIdx.x % PL;
    g.ly = threadIdx.x / PL;
    const int x0 = blockIdx.x * T - H, y0 = blockIdx.y * T - H;
    g.gx = x0 + g.lx;
    g.gy = y0 + g.ly;
    g.inside = g.gx >= 0 && g.gx < N && g.gy >= 0 && g.gy < N;
    g.i = g.inside ? g.gy * N + g.gx : 0;
    g.owned = g.inside && g.lx >= H && g.lx < H + T && g.ly >= H && g.ly < H + T;
    int kv = 1 << 20;
    if (x0 > 0) kv = min(kv, g.lx);
    if (x0 + PL - 1 < N - 1) kv = min(kv, PL - 1 - g.lx);
    if (y0 > 0) kv = min(kv, g.ly);
    if (y0 + PL - 1 < N - 1) kv = min(kv, PL - 1 - g.ly);
    g.kvalid = g.inside ? kv : 0;
    const int dx[6] = {1, 1, 0, -1, -1, 0}, dy[6] = {0, 1, 1, 0, -1, -1};
    g.self = g.ly * PLD + g.lx;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        int nx = min(max(g.lx + dx[s], 0), PL - 1), ny = min(max(g.ly + dy[s], 0), PL - 1);
        g.nb[s] = ny * PLD + nx;
    }
    // a patch of PL^2 nodes that is no whole number of waves: the block is rounded up and the spare threads own no node --
    // they load nothing, never update, write no LDS slot (tile_spare) and only reach the barriers
    if (PL * PL % WAVE != 0 && threadIdx.x >= PL * PL) {
        g.inside = g.owned = false;
        g.i = 0;
        g.kvalid = 0;
        g.self = 0;
    }
    return g;
}

template <int PL>
__device__ __forceinline__ bool tile_spare() {
    return PL * PL % WAVE != 0 && threadIdx.x >= PL * PL;
}

// The waves of a 32-patch workgroup that hold owned nodes (FEMFCT_TILE_TRIM bit 1): a wave is two patch rows, the owned
// rows are H .. 31 - H -- four waves of sixteen at H = 12 and 13.  Every other lane carries the identity of the
// reductions that end the Jacobi launches, so these waves alone have something to publish; a wave of a border tile whose
// rows lie outside the mesh publishes the identity.
__host__ __device__ constexpr int tile_owning_waves(int H) { return (TILE_L - 1 - H) / 2 - H / 2 + 1; }
template <int H>
__device__ __forceinline__ int tile_owning_wave() {       // 0 .. tile_owning_waves(H) - 1, or -1; uniform over the wave
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE) - H / 2;
    return w < tile_owning_waves(H) ? w : -1;             // (w < 0 is -1 or below already)
}

// ---- lean sweep loops (LEAN = 1, FEMFCT_TILE_LEAN) ----------------------------------------------------
// The same sweeps with three pieces of work taken out of the loop: the node's own value stays in a register (the
// thread computed it one sweep earlier), the two LDS buffers are addressed statically (the loop is unrolled by two:
// neighbour addresses are loop-invariant registers, the buffer is an immediate offset), and a node sweeps only while
// the owned tile can still see the result: a node at max-norm distance d from the tile influences it through sweep
// K - 1 - d at the latest.  A node live in sweep k has neighbours that were live in sweep k - 1 (their kvalid and
// their K - d are lower by one at most), so every value it reads was written into the buffer it reads from; nodes
// that never update (outside the mesh) are read from both buffers, which therefore both start with the input.
// Operands and their order are those of the LEAN = 0 loops: the owned values are the same bits.
template <int H, int PL = TILE_L>
__device__ __forceinline__ int tile_dist(const TileGeom& g) {
    constexpr int T = PL - 2 * H;
    const int ddx = max(max(H - g.lx, g.lx - (H + T - 1)), 0), ddy = max(max(H - g.ly, g.ly - (H + T - 1)), 0);
    return max(ddx, ddy);
}

// CONE (LEAN = 2, FEMFCT_TILE_CONE): the distance of the stencil's own graph instead of the max-norm.  The six
// neighbours are E, NE, N, W, SW, S, so one step along (1, 1) is one sweep and one step along (1, -1) is two: k sweeps
// reach a hexagon, and the NW and SE corners of the patch lie outside the owned tile's cone.  With ex, ey the signed
// excess beyond the tile, d = max(|ex|, |ey|) where they agree in sign and |ex| + |ey| where they do not.  d changes
// by at most one along each of the six slots, which is all the argument above uses.  Beside the liveness the cone
// also decides what a thread loads: the matrix row only where the node will ever be live, the iterate only where a
// live node reads it (d <= K); the others put the zeros of their defaults into LDS.
template <int H, int PL = TILE_L>
__device__ __forceinline__ int tile_hexdist(const TileGeom& g) {
    constexpr int T = PL - 2 * H;
    const int ex = g.lx - min(max(g.lx, H), H + T - 1), ey = g.ly - min(max(g.ly, H), H + T - 1);
    return max(max(abs(ex), abs(ey)), abs(ex - ey));      // (|ex - ey| is |ex| + |ey| where the signs differ, and no more than the larger where not)
}

template <int H, int LEAN, int PL = TILE_L>
__device__ __forceinline__ int lean_dist(const TileGeom& g) {
    if constexpr (LEAN == 2) return tile_hexdist<H, PL>(g);
    else return tile_dist<H, PL>(g);
}

struct LeanAddr {
    const double* n0[6];   // the six neighbours in buffer 0; buffer 1 lies PL * (PL + 1) doubles further
    double* me0;           // the node itself in buffer 0
};

template <int PL>
__device__ __forceinline__ LeanAddr lean_addr(double (*bufs)[PL * (PL + 1)], const TileGeom& g) {
    LeanAddr a;
    a.me0 = &bufs[0][g.self];
#pragma unroll
    for (int s = 0; s < 6; ++s) a.n0[s] = &bufs[0][g.nb[s]];
    return a;
}

// K Jacobi sweeps on two initialised buffers (xs[0] = xs[1] = input, barrier passed); returns the node's last iterate.
// BUF (0 / 1): the buffer a sweep reads; it writes the other one.  LAST: sweep K - 1, whose input's residual is taken
// (the last sweep is peeled off the loop, so the others carry no residual arithmetic).
template <int BUF, int LAST>
__device__ __forceinline__ void lean_jacobi_sweep(const LeanAddr& a, bool live, bool owned, const double* lv, double dg,
                                                  double rdg, double bv, double& xo, double& rmax) {
    constexpr int RD = BUF * TILE_L * TILE_LD, WR = (1 - BUF) * TILE_L * TILE_LD;
    if (live) {
        double acc = bv;
#pragma unroll
        for (int s = 0; s < 6; ++s) acc = fma(-lv[s], a.n0[s][RD], acc);
        if (LAST && owned) rmax = nan_max(rmax, fabs(acc - dg * xo));
        xo = acc * rdg;
        a.me0[WR] = xo;
    }
    __syncthreads();
}

__device__ __forceinline__ double lean_jacobi(const LeanAddr& a, int klive, int K, bool owned, const double* lv, double dg,
                                              double rdg, double bv, double xi, double& rmax) {
    double xo = xi;
    int k = 0;
    for (; k + 2 < K; k += 2) {
        lean_jacobi_sweep<0, 0>(a, k < klive, owned, lv, dg, rdg, bv, xo, rmax);
        lean_jacobi_sweep<1, 0>(a, k + 1 < klive, owned, lv, dg, rdg, bv, xo, rmax);
    }
    if (k + 1 < K) {
        lean_jacobi_sweep<0, 0>(a, k < klive, owned, lv, dg, rdg, bv, xo, rmax);
        lean_jacobi_sweep<1, 1>(a, k + 1 < klive, owned, lv, dg, rdg, bv, xo, rmax);
    } else if (k < K) {
        lean_jacobi_sweep<0, 1>(a, k < klive, owned, lv, dg, rdg, bv, xo, rmax);
    }
    return xo;
}

// One Chebyshev iteration of the three-term recurrence on two buffers of y_mid (ym, yo: the node's own y_mid and
// y_old, rotated in registers).
template <int BUF, int PL = TILE_L>
__device__ __forceinline__ void lean_cheb_iter(const LeanAddr& a, bool live, const double* mv, double md, double rmd, double bv,
                                               double wk, double& ym, double& yo) {
    constexpr int RD = BUF * PL * (PL + 1), WR = (1 - BUF) * PL * (PL + 1);
    if (live) {
        double acc = md * ym;
#pragma unroll
        for (int s = 0; s < 6; ++s) acc = fma(mv[s], a.n0[s][RD], acc);
        const double z = (bv - acc) * rmd;
        const double yn = wk * (z + ym - yo) + yo;
        yo = ym;
        ym = yn;
        a.me0[WR] = yn;
    }
    __syncthreads();
}

// BIG = 1: grids with more workgroups than in-kernel partials (bandwidth regime); the residual maxima
// go through k_reduce_resid.  A template parameter so that profiles list the two regimes separately.
// TRIM (FEMFCT_TILE_TRIM, lean loops only): bit 1 (deferred-test launches) -- the launch ends with its owning waves
// (tile_owning_waves: no block reduction, one partk slot per owning wave); bit 8 -- write-through output stores (TILE_OUT).
// 0 is the kernel as it was.
template <int H, int EXACT, int BIG, int LEAN, int TRIM = 0>
__global__ void __launch_bounds__(STRIP_T)
k_tile_jacobi(int n, int N, const double* __restrict__ L_, const double* __restrict__ b_, double* __restrict__ xa_,
              double* __restrict__ xb_, double* __restrict__ part, StepCtl* __restrict__ ctl_, int launch, int K,
              int g_build, double rel_tol, double* __restrict__ bigpart, double* __restrict__ partk, int bn_launch,
              int defer) {
    constexpr int W = 7;
    static_assert(!TRIM || (LEAN == 1 && !BIG), "trimmed launches: lean loops");
    static_assert(!(TRIM & 1) || !EXACT, "owning-wave epilogue: deferred test");
    __shared__ double xs[2][TILE_L * TILE_LD];
    __shared__ double smem[96];
    const int bz = blockIdx.z;
    StepCtl* ctl = ctl_ + bz;
    if (!defer && ctl->done) return;       // (defer: nothing sets `done` before this launch -- one dependent round trip less)
    double* p = part + (int64_t)bz * 4 * FEMFCT_MAX_PARTIALS;
    const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
    double bnorm;
    // ||b||, min row sum: reduced from the partials of the kernel that built L (k_build_low before launch 0,
    // or the fused k_tile_build_jacobi = launch 0 itself, then bn_launch = 1); launch >= 1 also tests the
    // residual the previous launch left.  In the fused case all three come out of one reduction pass.
    double rmax_prev = 0.0;
    bool have_rmax = false;
    // defer: a later launch of a solve of <= 4 launches whose first launch built the operator -- nothing is reduced and nothing
    // tested here (the test of launch 0's residual practically never passes; waiting for its partials costs this launch
    // ~2 us of its ~10); workgroup 0 of k_tile_dudt_cheb reduces everything at once (solve_ctl.h, deferred_test_*)
    if (defer) {
        bnorm = 0.0;
    } else if (launch == bn_launch) {
        double rsmin = INFINITY;
        bnorm = 0.0;
        if (!BIG && launch > 0 && g_build == nwg) {
            const double* pr = p + ((launch - 1) & 1) * FEMFCT_MAX_PARTIALS;
            for (int k = threadIdx.x; k < nwg; k += blockDim.x) {
                bnorm = nan_max(bnorm, p[2 * FEMFCT_MAX_PARTIALS + k]);
                rmax_prev = nan_max(rmax_prev, pr[k]);
                rsmin = nan_min(rsmin, p[3 * FEMFCT_MAX_PARTIALS + k]);
            }
            block_reduce_max_max_min(bnorm, rmax_prev, rsmin, smem);
            have_rmax = true;
        } else {
            bnorm = reduce_partials(p + 2 * FEMFCT_MAX_PARTIALS, g_build, OpMax(), 0.0, smem);
            rsmin = reduce_partials(p + 3 * FEMFCT_MAX_PARTIALS, g_build, OpMin(), INFINITY, smem);
        }
        if (wg == 0 && threadIdx.x == 0) {
            ctl->bnorm = bnorm;
            ctl->min_rowsum = rsmin;
            if (!(rsmin > 0.0)) ctl->flags |= FEMFCT_FLAG_MMATRIX_ROWSUM;
        }
    } else {
        bnorm = ctl->bnorm;
    }
    if (launch > 0 && !defer) {
        double rmax = have_rmax ? rmax_prev
                      : BIG   ? ctl->rs[(launch - 1) & 1]
                              : reduce_partials(p + ((launch - 1) & 1) * FEMFCT_MAX_PARTIALS, nwg, OpMax(), 0.0, smem);
        if (rmax <= rel_tol * bnorm) {
            if (wg == 0 && threadIdx.x == 0) {
                ctl->done = 1; ctl->parity = launch & 1; ctl->iters = launch * K; ctl->flags |= FEMFCT_FLAG_COARSE_ITERS;
                ctl->resid = bnorm != 0.0 ? rmax / bnorm : 0.0;
            }
            return;
        }
    }
    const int64_t moff = (int64_t)bz * W * n, voff = (int64_t)bz * n;
    const double* L = L_ + moff;
    const double* xin = ((launch & 1) ? xb_ : xa_) + voff;
    double* xout = ((launch & 1) ? xa_ : xb_) + voff;
    TILE_STAMP_BEGIN(H * TILE_L + H);
    const TileGeom g = tile_geom<TILE_L - 2 * H, H>(N);
    constexpr bool CONE = LEAN == 2;
    double lv[W - 1], dg = 1.0, rdg = 1.0, bv = 0.0, xi = 0.0;
#pragma unroll
    for (int s = 0; s < W - 1; ++s) lv[s] = 0.0;
    if constexpr (CONE) {
        // the row only where the node is ever live, the iterate only where a live node reads it
        const int dist = tile_hexdist<H>(g);
        if (g.inside && ((dist < K && g.kvalid > 0) || g.owned)) {
            dg = L[g.i];
            rdg = 1.0 / dg;
#pragma unroll
            for (int s = 1; s < W; ++s) lv[s - 1] = L[(int64_t)s * n + g.i];
            bv = b_[voff + g.i];
        }
        if (g.inside && dist <= K) xi = xin[g.i];
    } else if (g.inside) {
        dg = L[g.i];
        rdg = 1.0 / dg;
#pragma unroll
        for (int s = 1; s < W; ++s) lv[s - 1] = L[(int64_t)s * n + g.i];
        bv = b_[voff + g.i];
        xi = xin[g.i];
    }
    xs[0][g.self] = xi;
    if (LEAN) xs[1][g.self] = xi;          // nodes that never update are read from both buffers
    __syncthreads();
    TILE_STAMP_LOADED();
    double rmax = 0.0;
    int cur = 0;
    [[maybe_unused]] double xo = xi;                             // LEAN: own iterate, a register, never re-read
    [[maybe_unused]] const int klive = min(g.kvalid, K - lean_dist<H, LEAN>(g));   // LEAN: sweeps whose result the owned tile can still see
    [[maybe_unused]] const LeanAddr a = lean_addr<TILE_L>(xs, g);
    if (!EXACT) {
        if constexpr (LEAN) xo = lean_jacobi(a, klive, K, g.owned, lv, dg, rdg, bv, xi, rmax);
        else
        for (int k = 0; k < K; ++k) {
            const double* c = xs[cur];
            double xn = c[g.self];
            if (k < g.kvalid) {
                double acc = bv;
#pragma unroll
                for (int s = 0; s < W - 1; ++s) acc = fma(-lv[s], c[g.nb[s]], acc);
                if (k == K - 1 && g.owned) rmax = nan_max(rmax, fabs(acc - dg * xn));
                xn = acc * rdg;
            }
            xs[cur ^ 1][g.self] = xn;
            __syncthreads();
            cur ^= 1;
        }
        TILE_STAMP_SWEPT();
    } else {
        // last launch of the budget, optional: log the residual of every sweep's input so that the
        // host learns the exact sweep count (fully unrolled: per-sweep values stay in registers)
        double rk[H];
#pragma unroll
        for (int k = 0; k < H; ++k) {
            rk[k] = 0.0;
            if (k < K) {
                if constexpr (LEAN) {
                    const int rd = (k & 1) * TILE_L * TILE_LD, wr = ((k + 1) & 1) * TILE_L * TILE_LD;
                    if (k < klive) {
                        double acc = bv;
#pragma unroll
                        for (int s = 0; s < W - 1; ++s) acc = fma(-lv[s], a.n0[s][rd], acc);
                        if (g.owned) rk[k] = fabs(acc - dg * xo);
                        if (k == K - 1) rmax = nan_max(rmax, rk[k]);
                        xo = acc * rdg;
                        a.me0[wr] = xo;
                    }
                    __syncthreads();
                    continue;
                }
                const double* c = xs[cur];
                double xn = c[g.self];
                if (k < g.kvalid) {
                    double acc = bv;
#pragma unroll
                    for (int s = 0; s < W - 1; ++s) acc = fma(-lv[s], c[g.nb[s]], acc);
                    if (g.owned) rk[k] = fabs(acc - dg * xn);
                    if (k == K - 1) rmax = nan_max(rmax, rk[k]);
                    xn = acc * rdg;
                }
                xs[cur ^ 1][g.self] = xn;
                __syncthreads();
                cur ^= 1;
            }
        }
        __shared__ double sk[H][STRIP_T / WAVE];
        const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
        for (int k = 0; k < H; ++k) {
            double v = wave_reduce(rk[k], OpMax());
            if (lane == 0) sk[k][wid] = v;
        }
        __syncthreads();
        if (threadIdx.x < H) {
            double v = 0.0;
            for (int w = 0; w < STRIP_T / WAVE; ++w) v = nan_max(v, sk[threadIdx.x][w]);
            partk[((int64_t)bz * 16 + threadIdx.x) * FEMFCT_MAX_PARTIALS + wg] = v;
        }
    }
    if (g.owned) TILE_OUT(xout[g.i], LEAN ? xo : xs[cur][g.self]);        // LEAN: no LDS read-back
    if constexpr (TRIM & 1) {
        // deferred test only (the launcher sees to it): one slot of this launch's partk row per owning wave
        const int ow = tile_owning_wave<H>();
        if (ow >= 0) {
            rmax = wave_reduce(rmax, OpMax());
            if (threadIdx.x % WAVE == 0)
                partk[((int64_t)bz * 16 + launch) * FEMFCT_MAX_PARTIALS + wg * tile_owning_waves(H) + ow] = rmax;
        }
        TILE_STAMP_END(1);
        return;
    }
    rmax = block_reduce(rmax, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) {
        if (BIG) bigpart[(int64_t)bz * nwg + wg] = rmax;
        else if (defer) partk[((int64_t)bz * 16 + launch) * FEMFCT_MAX_PARTIALS + wg] = rmax;   // one slot per launch
        else p[(launch & 1) * FEMFCT_MAX_PARTIALS + wg] = rmax;
    }
    TILE_STAMP_END(1);
}

// Launch 0 of the low-order solve with the construction of the low-order operator folded in
// (what k_build_low does, helpers.py:1769-1780, same expressions in the same order => bitwise the same
// L, D, b): every thread builds the row of its patch node from A (a_ji comes from the neighbour thread
// through LDS, three slots at a time), the tile's owned rows are stored for the later launches / the
// limiter, then K Jacobi sweeps run as in k_tile_jacobi.  Saves one dependent launch per time step.
// PRE = 1: the operator was built before the sweep (k_low_seq): A_ref is the L_k sequence, read instead of built (no
// a_ji exchange, no D store: the limiter reads D_k from the sequence); the owned rows of L still go to L_ for launch 1.
// TRIM (FEMFCT_TILE_TRIM, lean loops): bit 1 (solves whose test is deferred) -- the three partials per owning wave instead
// of per workgroup, no block reduction; bit 8 -- write-through output stores (TILE_OUT).  0 is the kernel as it was.
template <int H, int PRE, int LEAN, int TRIM = 0>
__global__ void __launch_bounds__(STRIP_T)
k_tile_build_jacobi(int n, int N, MatRef A_ref, const double* __restrict__ N_, int nshared,
                    VecRef rhs_ref, int64_t rhs_bstride, VecRef u_ref, int64_t u_bstride,
                    const double* __restrict__ ml, double dt, double* __restrict__ L_, double* __restrict__ D_,
                    double* __restrict__ b_, double* __restrict__ xb_, double* __restrict__ part,
                    StepCtl* __restrict__ ctl_, int K) {
    constexpr int W = 7;
    static_assert(!TRIM || LEAN == 1, "trimmed launches: lean loops");
    __shared__ double xs[2][TILE_L * TILE_LD];
    __shared__ double as[PRE ? 1 : 3][TILE_L * TILE_LD];
    __shared__ double smem[96];
    const int bz = blockIdx.z;
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    double* p = part + (int64_t)bz * 4 * FEMFCT_MAX_PARTIALS;
    if (wg == 0 && threadIdx.x == 0) {
        StepCtl* c = ctl_ + bz;
        c->flags = 0; c->iters = 0; c->done = 0; c->parity = 0; c->resid = 0.0; c->bnorm = 0.0;
        c->min_rowsum = 0.0;
    }
    const int64_t moff = (int64_t)bz * W * n, voff = (int64_t)bz * n;
    const double* A = mat_ptr(A_ref, bz);
    const double* Nm = N_ ? N_ + (nshared ? 0 : moff) : nullptr;
    const double* rhs = vec_ptr(rhs_ref);
    if (rhs) rhs += bz * rhs_bstride;
    const double* u = vec_ptr(u_ref) + bz * u_bstride;
    TILE_STAMP_BEGIN(H * TILE_L + H);
    const TileGeom g = tile_geom<TILE_L - 2 * H, H>(N);
    double lv[W - 1], dv[W - 1], dsum = 0.0, rs = 0.0;
    double dg = 1.0, rdg = 1.0, bv = 0.0, xi = 0.0;
    if constexpr (PRE) {
        // the rows k_low_seq built (bitwise those of the branch below); the row sum in the same order
#pragma unroll
        for (int s = 0; s < W - 1; ++s) lv[s] = 0.0;
        if constexpr (LEAN == 2) {
            // CONE: the row, M_L and the rhs only where the node is ever live, u^n only where a live node reads it
            const int dist = tile_hexdist<H>(g);
            const bool row = g.inside && ((dist < K && g.kvalid > 0) || g.owned);
            if (row) {
                dg = A[g.i];
#pragma unroll
                for (int s = 1; s < W; ++s) lv[s - 1] = A[(int64_t)s * n + g.i];
            }
#pragma unroll
            for (int s = 0; s < W - 1; ++s) rs += lv[s];
            if (g.inside && dist <= K) xi = u[g.i];
            if (row) {
                const double mli = ml[g.i];
                rs += dg;
                rdg = 1.0 / dg;
                bv = mli * xi + (rhs ? dt * rhs[g.i] : 0.0);
            }
        } else {
            if (g.inside) {
                dg = A[g.i];
#pragma unroll
                for (int s = 1; s < W; ++s) lv[s - 1] = A[(int64_t)s * n + g.i];
            }
#pragma unroll
            for (int s = 0; s < W - 1; ++s) rs += lv[s];
            if (g.inside) {
                const double mli = ml[g.i];
                rs += dg;
                rdg = 1.0 / dg;
                xi = u[g.i];
                bv = mli * xi + (rhs ? dt * rhs[g.i] : 0.0);
            }
        }
    } else {
        // neighbour s exists in the grid (otherwise the ELL slot is padding: column = row, value 0)
        const int dx[6] = {1, 1, 0, -1, -1, 0}, dy[6] = {0, 1, 1, 0, -1, -1};
        bool ex[W - 1];
#pragma unroll
        for (int s = 0; s < W - 1; ++s) {
            const int nx = g.gx + dx[s], ny = g.gy + dy[s];
            ex[s] = g.inside && nx >= 0 && nx < N && ny >= 0 && ny < N;
        }
        double av[W - 1], at[W - 1], a0 = 0.0;
#pragma unroll
        for (int s = 0; s < W - 1; ++s) av[s] = 0.0;
        if (g.inside) {
            a0 = A[g.i];
#pragma unroll
            for (int s = 1; s < W; ++s) av[s - 1] = A[(int64_t)s * n + g.i];
        }
        // a_ji of slot s lives in row j at the opposite slot: slots E,NE,N <-> W,SW,S
#pragma unroll
        for (int s = 0; s < 3; ++s) as[s][g.self] = av[s + 3];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 3; ++s) at[s] = as[s][g.nb[s]];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 3; ++s) as[s][g.self] = av[s];
        __syncthreads();
#pragma unroll
        for (int s = 3; s < 6; ++s) at[s] = as[s - 3][g.nb[s]];
#pragma unroll
        for (int s = 0; s < W - 1; ++s) {
            const double a = av[s];
            const double d = ex[s] ? fmax(0.0, fmax(a, at[s])) : 0.0;   // d_ij = max(0, a_ij, a_ji)
            dsum += d;
            double l = dt * (a - d);
            if (Nm && g.inside) l += dt * Nm[(int64_t)(s + 1) * n + g.i];
            lv[s] = l;
            dv[s] = d;
            rs += l;
        }
        if (g.inside) {
            const double mli = ml[g.i];
            double ld = mli + dt * (a0 + dsum);                         // d_ii = -sum_j d_ij
            if (Nm) ld += dt * Nm[g.i];
            rs += ld;
            dg = ld;
            rdg = 1.0 / dg;
            xi = u[g.i];
            bv = mli * xi + (rhs ? dt * rhs[g.i] : 0.0);
        }
    }
    double bmax = 0.0, rsmin = INFINITY;
    if (g.owned) {
        double* L = L_ + moff;
        TILE_OUT(L[g.i], dg);
#pragma unroll
        for (int s = 1; s < W; ++s) TILE_OUT(L[(int64_t)s * n + g.i], lv[s - 1]);
        if constexpr (!PRE) {
            double* D = D_ + moff;
            D[g.i] = -dsum;
#pragma unroll
            for (int s = 1; s < W; ++s) D[(int64_t)s * n + g.i] = dv[s - 1];
        }
        TILE_OUT(b_[voff + g.i], bv);
        bmax = fabs(bv);
        rsmin = rs;
    }
    xs[0][g.self] = xi;
    if (LEAN) xs[1][g.self] = xi;          // nodes that never update are read from both buffers
    __syncthreads();
    TILE_STAMP_LOADED();
    double rmax = 0.0;
    int cur = 0;
    [[maybe_unused]] double xo = xi;
    if constexpr (LEAN) xo = lean_jacobi(lean_addr<TILE_L>(xs, g), min(g.kvalid, K - lean_dist<H, LEAN>(g)), K, g.owned, lv, dg, rdg, bv, xi, rmax);
    else
    for (int k = 0; k < K; ++k) {
        const double* c = xs[cur];
        double xn = c[g.self];
        if (k < g.kvalid) {
            double acc = bv;
#pragma unroll
            for (int s = 0; s < W - 1; ++s) acc = fma(-lv[s], c[g.nb[s]], acc);
            if (k == K - 1 && g.owned) rmax = nan_max(rmax, fabs(acc - dg * xn));
            xn = acc * rdg;
        }
        xs[cur ^ 1][g.self] = xn;
        __syncthreads();
        cur ^= 1;
    }
    TILE_STAMP_SWEPT();
    if (g.owned) TILE_OUT(xb_[voff + g.i], LEAN ? xo : xs[cur][g.self]);
    if constexpr (TRIM & 1) {
        // deferred test only (the launcher sees to it): deferred_test_load alone reads these, slot by slot
        const int ow = tile_owning_wave<H>();
        if (ow >= 0) {
            rmax = wave_reduce(rmax, OpMax());
            bmax = wave_reduce(bmax, OpMax());
            rsmin = wave_reduce(rsmin, OpMin());
            if (threadIdx.x % WAVE == 0) {
                const int slot = wg * tile_owning_waves(H) + ow;
                p[slot] = rmax;
                p[2 * FEMFCT_MAX_PARTIALS + slot] = bmax;
                p[3 * FEMFCT_MAX_PARTIALS + slot] = rsmin;
            }
        }
        TILE_STAMP_END(0);
        return;
    }
    block_reduce_max_max_min(rmax, bmax, rsmin, smem);
    if (threadIdx.x == 0) {
        p[wg] = rmax;
        p[2 * FEMFCT_MAX_PARTIALS + wg] = bmax;
        p[3 * FEMFCT_MAX_PARTIALS + wg] = rsmin;
    }
    TILE_STAMP_END(0);
}

// The low-order operator of every entry of a pre-assembled sequence, once before the sweep (FEMFCT_PREBUILD_LOW):
// L_k = M_L + dt (A_k - D_k) and D_k depend on the control only.  The expressions and their order are those of
// k_tile_build_jacobi (no non-flux matrix), so the bits are the same; a_ji is read from the neighbour's row.
// Structured mesh in vertex order; blockIdx.y = sequence entry (as k_ops_solidbody writes them).
__global__ void __launch_bounds__(256)
k_low_seq(int n, int N, const double* __restrict__ A_, const double* __restrict__ ml, double dt, double* __restrict__ L_,
          double* __restrict__ D_) {
    constexpr int W = 7;
    const int64_t off = (int64_t)blockIdx.y * W * n;
    const double* A = A_ + off;
    double* L = L_ + off;
    double* D = D_ + off;
    const int dx[6] = {1, 1, 0, -1, -1, 0}, dy[6] = {0, 1, 1, 0, -1, -1};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int gx = i % N, gy = i / N;
        double av[W - 1], at[W - 1];
        bool ex[W - 1];
        const double a0 = A[i];
#pragma unroll
        for (int s = 0; s < W - 1; ++s) {
            const int nx = gx + dx[s], ny = gy + dy[s];
            ex[s] = nx >= 0 && nx < N && ny >= 0 && ny < N;
            av[s] = A[(int64_t)(s + 1) * n + i];
            // a_ji of slot s lives in row j at the opposite slot: slots E,NE,N <-> W,SW,S
            at[s] = ex[s] ? A[(int64_t)(s < 3 ? s + 4 : s - 2) * n + ny * N + nx] : 0.0;
        }
        double dsum = 0.0;
#pragma unroll
        for (int s = 0; s < W - 1; ++s) {
            const double a = av[s];
            const double d = ex[s] ? fmax(0.0, fmax(a, at[s])) : 0.0;   // d_ij = max(0, a_ij, a_ji)
            dsum += d;
            L[(int64_t)(s + 1) * n + i] = dt * (a - d);
            D[(int64_t)(s + 1) * n + i] = d;
        }
        L[i] = ml[i] + dt * (a0 + dsum);                                // d_ii = -sum_j d_ij
        D[i] = -dsum;
    }
}

// one block per batch member: max over the residual partials of a fused launch on a large grid
__global__ void __launch_bounds__(STRIP_T)
k_reduce_resid(const double* __restrict__ bigpart, int64_t count, StepCtl* __restrict__ ctl_, int launch) {
    __shared__ double smem[32];
    const int bz = blockIdx.x;
    if (ctl_[bz].done) return;
    const double* q = bigpart + (int64_t)bz * count;
    double v = 0.0;
    for (int64_t k = threadIdx.x; k < count; k += blockDim.x) v = nan_max(v, q[k]);
    v = block_reduce(v, OpMax(), 0.0, smem);
    if (threadIdx.x == 0) ctl_[bz].rs[launch & 1] = v;
}

template <int H, int LEAN>
__global__ void __launch_bounds__(STRIP_T)
k_tile_cheb(int n, int N, const double* __restrict__ M, const double* __restrict__ b_, const double* __restrict__ ymid_,
            const double* __restrict__ yold_, double* __restrict__ omid_, double* __restrict__ oold_, int K,
            CheOmegas om, double md_scale, ChebIO cio) {
    constexpr int W = 7;
    __shared__ double ys[LEAN ? 2 : 3][TILE_L * TILE_LD];
    const int64_t voff = (int64_t)blockIdx.z * n;
    if (cio.mat) M = cio.mat + (int64_t)blockIdx.z * cio.mat_bs;
    if (cio.scale_dev) md_scale = cio.scale_dev[blockIdx.z];
    const double* omd = cio.om_dev ? cio.om_dev + (int64_t)blockIdx.z * cio.om_bs + cio.k0 : nullptr;
    if (cio.mid_ref.base) ymid_ = vec_ptr(cio.mid_ref) + (int64_t)blockIdx.z * cio.mid_bs - voff;
    if (cio.out_ref.base) omid_ = const_cast<double*>(vec_ptr(cio.out_ref)) + (int64_t)blockIdx.z * cio.out_bs - voff;
    const TileGeom g = tile_geom<TILE_L - 2 * H, H>(N);
    constexpr bool CONE = LEAN == 2;
    double mv[W - 1], md = 1.0, rmd = 1.0, bv = 0.0, ym = 0.0, yo = 0.0;
#pragma unroll
    for (int s = 0; s < W - 1; ++s) mv[s] = 0.0;
    if constexpr (CONE) {
        // the row and y_old only where the node is ever live, y_mid only where a live node reads it
        const int dist = tile_hexdist<H>(g);
        if (g.inside && ((dist < K && g.kvalid > 0) || g.owned)) {
            md = M[g.i];
            rmd = 1.0 / (md_scale * md);
#pragma unroll
            for (int s = 1; s < W; ++s) mv[s - 1] = M[(int64_t)s * n + g.i];
            bv = b_[voff + g.i];
            if (yold_) yo = yold_[voff + g.i];
        }
        if (g.inside && dist <= K && ymid_) ym = ymid_[voff + g.i];
    } else if (g.inside) {
        md = M[g.i];
        rmd = 1.0 / (md_scale * md);
#pragma unroll
        for (int s = 1; s < W; ++s) mv[s - 1] = M[(int64_t)s * n + g.i];
        bv = b_[voff + g.i];
        if (ymid_) ym = ymid_[voff + g.i];
        if (yold_) yo = yold_[voff + g.i];
    }
    if constexpr (LEAN) {
        // both buffers hold y_mid; y_mid and y_old of the node itself stay in ym, yo
        ys[0][g.self] = ym;
        ys[1][g.self] = ym;
        __syncthreads();
        const int klive = min(g.kvalid, K - lean_dist<H, LEAN>(g));
        const LeanAddr a = lean_addr<TILE_L>(ys, g);
        int k = 0;
        for (; k + 1 < K; k += 2) {
            lean_cheb_iter<0>(a, k < klive, mv, md, rmd, bv, omd ? omd[k] : om.w[k], ym, yo);
            lean_cheb_iter<1>(a, k + 1 < klive, mv, md, rmd, bv, omd ? omd[k + 1] : om.w[k + 1], ym, yo);
        }
        if (k < K) lean_cheb_iter<0>(a, k < klive, mv, md, rmd, bv, omd ? omd[k] : om.w[k], ym, yo);
        if (g.owned) {
            omid_[voff + g.i] = ym;
            if (oold_) oold_[voff + g.i] = yo;
        }
        return;
    }
    ys[0][g.self] = yo;
    ys[1][g.self] = ym;
    __syncthreads();
    int io = 0, im = 1, in_ = 2;
    for (int k = 0; k < K; ++k) {
        const double* ymd = ys[im];
        const double ymv = ymd[g.self];
        double yn = ymv;
        if (k < g.kvalid) {
            double acc = md * ymv;
#pragma unroll
            for (int s = 0; s < W - 1; ++s) acc = fma(mv[s], ymd[g.nb[s]], acc);
            const double z = (bv - acc) * rmd;
            const double yov = ys[io][g.self];
            const double wk = omd ? omd[k] : om.w[k];
            yn = wk * (z + ymv - yov) + yov;
        }
        ys[in_][g.self] = yn;
        __syncthreads();
        int t = io; io = im; im = in_; in_ = t;
    }
    if (g.owned) {
        omid_[voff + g.i] = ys[im][g.self];
        if (oold_) oold_[voff + g.i] = ys[io][g.self];
    }
}


// flux + Zalesak limiter + explicit correction in one launch (helpers.py:1818-1870): a 12 x 12
// tile with a halo of two rings (16 x 16 patch, 256 threads) (R+- of the first ring needs u_L, du/dt of the second);
// F_ij stays in registers, R+- goes through LDS.
#define FL_H 2
// (two 1024-thread workgroups per CU need <= 64 VGPRs: the second launch-bound argument is waves per SIMD)
// LDS slot of neighbour s of this thread's node (clamped into the patch, as TileGeom::nb), recomputed from the thread
// index at every use: kept in registers across the limiter's three phases the six slots are what the 32-patch variant
// (64-VGPR limit) spills -- 12 bytes per lane, 66 MB of scratch traffic per launch at 2049^2
template <int PL>
__device__ __forceinline__ int fl_nb(int s) {
    const int lx = threadIdx.x % PL, ly = threadIdx.x / PL;
    const int dx = (s == 0 || s == 1) ? 1 : (s == 3 || s == 4) ? -1 : 0;
    const int dy = (s == 1 || s == 2) ? 1 : (s == 4 || s == 5) ? -1 : 0;
    return min(max(ly + dy, 0), PL - 1) * (PL + 1) + min(max(lx + dx, 0), PL - 1);
}

template <int FL_L, int GEOM, int HALFD>   // patch edge: 16 (256 threads, many workgroups: small meshes) or 32 (less halo re-reading)
__global__ void __launch_bounds__(FL_L * FL_L, FL_L == 32 ? 8 : 1)
k_tile_flux_limit(int n, int N, double h, const double* __restrict__ M, const double* __restrict__ D_,
                  const double* __restrict__ ulow_, const double* __restrict__ du_, const double* __restrict__ ml,
                  double dt, VecRef out_ref, int64_t out_bstride, EndArgs e) {
    constexpr int W = 7;
    constexpr int FL_LD = FL_L + 1, FL_T = FL_L - 2 * FL_H;
    __shared__ double su[FL_L * FL_LD], sd[FL_L * FL_LD], srp[FL_L * FL_LD], srm[FL_L * FL_LD];
    __shared__ double sdf[HALFD ? 3 : 1][HALFD ? FL_L * FL_LD : 1];   // HALFD: the forward slots (E, NE, N) of D
    // The step end is folded in for the 16-patch only (meshes up to 512^2, where a launch counts); the 32-patch runs at
    // its 64-VGPR limit (two 1024-thread workgroups per CU) and every spilled dword there is 44 MB of scratch traffic
    // at 2049^2 -- its step end stays a separate tiny launch (femfct_enqueue_tile_flux_limit reports fuse_end back).
    if (FL_L == 16) step_log_early(e);
    const int bz = blockIdx.z;
    const int64_t moff = (int64_t)bz * W * n, voff = (int64_t)bz * n;
    const TileGeom g = tile_geom<FL_T, FL_H, FL_L>(N);
    double ui = 0.0, dui = 0.0, mli = 1.0, dfw[3] = {0.0, 0.0, 0.0};
    if (g.inside) { ui = ulow_[voff + g.i]; dui = du_[voff + g.i]; mli = ml[g.i]; }
    if (HALFD) {
        // d_ij is stored once per edge, in the row whose slot towards the neighbour is E, NE or N (k_build_low, half_d)
        if (g.inside) {
#pragma unroll
            for (int s = 0; s < 3; ++s) dfw[s] = D_[moff + (int64_t)(s + 1) * n + g.i];
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) sdf[s][g.self] = dfw[s];
    }
    su[g.self] = ui;
    sd[g.self] = dui;
    srp[g.self] = 1.0;
    srm[g.self] = 1.0;
    __syncthreads();
    double f[W - 1];
    // every inside node whose six neighbours are in the patch (or outside the grid) gets its fluxes
    const bool have = g.inside && g.kvalid >= 1;
    if (have) {
        double pp = 0.0, pm = 0.0, umax = ui, umin = ui;
        const int pc = (GEOM || HALFD) ? mass_edge_counts(g.gx, g.gy, N - 1) : 0;
        const double mq = (0.5 * h * h) / 12.0;
#pragma unroll
        for (int s = 1; s < W; ++s) {
            const int64_t idx = (int64_t)s * n + g.i;
            const int nbs = fl_nb<FL_L>(s - 1);
            const double uj = su[nbs];
            const double mij = GEOM ? (double)((pc >> (2 * (s - 1))) & 3) * mq : M[idx];
            double dij;
            if (HALFD) {
                // backward slots W, SW, S: the neighbour's forward entry (a neighbour outside the grid has none:
                // its clamped LDS slot aliases a patch node)
                const bool exists = ((pc >> (2 * (s - 1))) & 3) != 0;
                dij = s <= 3 ? sdf[s - 1][g.self] : (exists ? sdf[s - 4][nbs] : 0.0);   // (own entries re-read from LDS: six registers less across the barrier)
            } else {
                dij = D_[moff + idx];
            }
            const double fs = mij * (dui - sd[nbs]) + dij * (ui - uj);
            f[s - 1] = fs;
            pp += fmax(fs, 0.0);
            pm += fmin(fs, 0.0);
            // a clamped neighbour (outside the grid) has M = D = 0 and must not enter the bounds:
            // its LDS slot then aliases a patch node, so take it only when the coefficient is live
            const bool live = (mij != 0.0) || (dij != 0.0);
            umax = live ? fmax(umax, uj) : umax;
            umin = live ? fmin(umin, uj) : umin;
        }
        const double qp = umax - ui, qm = umin - ui;
        srp[g.self] = (pp != 0.0) ? fmin(1.0, mli * qp / (dt * pp)) : 1.0;
        srm[g.self] = (pm != 0.0) ? fmin(1.0, mli * qm / (dt * pm)) : 1.0;
    }
    __syncthreads();
    if (g.owned) {
        const double rpi = srp[g.self], rmi = srm[g.self];
        double fbar = 0.0;
#pragma unroll
        for (int s = 0; s < W - 1; ++s) {
            const double fs = f[s];
            const int nbs = fl_nb<FL_L>(s);
            const double a = (fs > 0.0) ? fmin(rpi, srm[nbs]) : fmin(rmi, srp[nbs]);
            fbar += a * fs;
        }
        double* out = const_cast<double*>(vec_ptr(out_ref)) + bz * out_bstride;
        out[g.i] = ui + dt * fbar / mli;
    }
    if (FL_L == 16) step_end_by_last_workgroup(e);
}

// The last <= 10 Chebyshev iterations of du/dt (helpers.py:175-184) and the whole limiter
// (helpers.py:1818-1870) in one launch: 8 x 8 tile + halo 12 (ten rings for the iterations, two for
// the limiter: R+- of the ring-1 neighbours).  du never goes to memory.  Same expressions in the same
// order as k_tile_cheb + k_tile_flux_limit => bitwise the same step.  Latency regime only.
// (LEAN = 1 compiles to 72 VGPRs when left alone; the waves-per-SIMD bound 8 holds it at the 64 of LEAN = 0, without scratch)
// PL (FEMFCT_TILE_FIT): the patch edge.  32 is the 8 x 8 tile; 30 is a 6 x 6 tile whose halo of 12 needs no more -- 15
// waves instead of 16 and more workgroups, chosen while each still gets a compute unit (femfct_tile_fit).  The block is
// PL^2 threads rounded up to whole waves; the spare threads own no node (tile_geom).
// TRIM (FEMFCT_TILE_TRIM, lean loops): bit 8 -- write-through output store (TILE_OUT).  0 is the kernel as it was.
template <int GEOM, int LEAN, int PL, int TRIM = 0>
__global__ void __launch_bounds__((PL * PL + WAVE - 1) / WAVE * WAVE, (LEAN && PL == TILE_L) ? 8 : 1)
k_tile_cheb_flux_limit(int n, int N, double h, const double* __restrict__ M, const double* __restrict__ b_,
                       const double* __restrict__ ymid_, const double* __restrict__ yold_, int K, CheOmegas om,
                       double md_scale, MatRef D_ref, const double* __restrict__ ulow_,
                       const double* __restrict__ ml, double dt, VecRef out_ref, int64_t out_bstride, EndArgs e) {
    constexpr int W = 7, HH = 12, PLD = PL + 1;
    constexpr bool CONE = LEAN == 2;
    static_assert(PL == TILE_L || LEAN, "fitted patches run the lean loops only");
    static_assert(!TRIM || LEAN == 1, "trimmed launches: lean loops");
    __shared__ double ys[LEAN ? 2 : 3][PL * PLD];
    __shared__ double su[PL * PLD], srp[PL * PLD], srm[PL * PLD];
    const int bz = blockIdx.z;
    const int64_t voff = (int64_t)bz * n;
    const double* D_ = mat_ptr(D_ref, bz);     // the step's D (one of the pre-built sequence, or the workspace's)
    TILE_STAMP_BEGIN(HH * PL + HH);
    const TileGeom g = tile_geom<PL - 2 * HH, HH, PL>(N);
    double mv[W - 1], dv[W - 1], md = 1.0, rmd = 1.0, bv = 0.0, ym = 0.0, yo = 0.0, ui = 0.0, mli = 1.0;
#pragma unroll
    for (int s = 0; s < W - 1; ++s) { mv[s] = 0.0; dv[s] = 0.0; }
    [[maybe_unused]] bool flux_node = false;
    if constexpr (CONE) {
        // the mass row, the rhs and y_old where the node iterates or takes fluxes (`have` and `klive` below), y_mid where
        // an iterating node or a flux reads it, u_L and M_L two rings out (the fluxes and their neighbours), D on the first ring
        const int dist = tile_hexdist<HH, PL>(g);
        flux_node = g.inside && g.kvalid >= K + 1 && dist <= 1;
        if (g.inside && (min(g.kvalid, K - max(dist - 2, 0)) > 0 || flux_node)) {
            md = M[g.i];
            rmd = 1.0 / (md_scale * md);
            if (GEOM) {
                const int pc = mass_edge_counts(g.gx, g.gy, N - 1);
                const double mq = (0.5 * h * h) / 12.0;
#pragma unroll
                for (int s = 1; s < W; ++s) mv[s - 1] = (double)((pc >> (2 * (s - 1))) & 3) * mq;
            } else {
#pragma unroll
                for (int s = 1; s < W; ++s) mv[s - 1] = M[(int64_t)s * n + g.i];
            }
            bv = b_[voff + g.i];
            yo = yold_[voff + g.i];
        }
        if (g.inside && max(dist - 2, 0) <= K) ym = ymid_[voff + g.i];
        if (g.inside && dist <= 2) {
            ui = ulow_[voff + g.i];
            mli = ml[g.i];
        }
    } else if (g.inside) {
        md = M[g.i];
        rmd = 1.0 / (md_scale * md);
        if (GEOM) {
            const int pc = mass_edge_counts(g.gx, g.gy, N - 1);
            const double mq = (0.5 * h * h) / 12.0;
#pragma unroll
            for (int s = 1; s < W; ++s) mv[s - 1] = (double)((pc >> (2 * (s - 1))) & 3) * mq;
        } else {
#pragma unroll
            for (int s = 1; s < W; ++s) mv[s - 1] = M[(int64_t)s * n + g.i];
        }
        bv = b_[voff + g.i];
        ym = ymid_[voff + g.i];
        yo = yold_[voff + g.i];
        ui = ulow_[voff + g.i];
        mli = ml[g.i];
    }
    if (!tile_spare<PL>()) {
        ys[0][g.self] = LEAN ? ym : yo;    // LEAN: both buffers hold y_mid, the node's own y_mid / y_old stay in ym, yo
        ys[1][g.self] = ym;
        su[g.self] = ui;
        srp[g.self] = 1.0;
        srm[g.self] = 1.0;
    }
    __syncthreads();
    TILE_STAMP_LOADED();
    step_log_early(e);        // (behind this kernel's own loads; its round trip is covered by the Chebyshev iterations)
    // D is first needed by the fluxes: requested behind the log copy (which waits for every load in flight) so that a
    // pre-built D_k, an HBM round trip behind the level counter, is covered by the iterations too
    if (g.inside && (!CONE || flux_node)) {
#pragma unroll
        for (int s = 1; s < W; ++s) dv[s - 1] = D_[(int64_t)s * n + g.i];
    }
    int io = 0, im = 1, in_ = 2;
    // fluxes where all six neighbours carry the final du (one ring inside the iterations' validity).  LEAN: only where
    // the owned tile reads R+- (its first ring); there the node and its six neighbours iterated to the end (their
    // kvalid is at least K), so the last buffer holds their final du.
    const bool have = g.inside && g.kvalid >= K + 1 && (!LEAN || lean_dist<HH, LEAN, PL>(g) <= 1);
    if constexpr (LEAN) {
        // the fluxes of the tile's first ring need du two rings out: a node stops iterating d - 2 iterations early
        const int klive = min(g.kvalid, K - max(lean_dist<HH, LEAN, PL>(g) - 2, 0));
        const LeanAddr a = lean_addr<PL>(ys, g);
        int k = 0;
        for (; k + 1 < K; k += 2) {
            lean_cheb_iter<0, PL>(a, k < klive, mv, md, rmd, bv, om.w[k], ym, yo);
            lean_cheb_iter<1, PL>(a, k + 1 < klive, mv, md, rmd, bv, om.w[k + 1], ym, yo);
        }
        if (k < K) lean_cheb_iter<0, PL>(a, k < klive, mv, md, rmd, bv, om.w[k], ym, yo);
        im = K & 1;                         // the buffer iteration K - 1 wrote (K = 0: either)
    } else
    for (int k = 0; k < K; ++k) {
        const double* ymd = ys[im];
        const double ymv = ymd[g.self];
        double yn = ymv;
        if (k < g.kvalid) {
            double acc = md * ymv;
#pragma unroll
            for (int s = 0; s < W - 1; ++s) acc = fma(mv[s], ymd[g.nb[s]], acc);
            const double z = (bv - acc) * rmd;
            const double yov = ys[io][g.self];
            yn = om.w[k] * (z + ymv - yov) + yov;
        }
        ys[in_][g.self] = yn;
        __syncthreads();
        int t = io; io = im; im = in_; in_ = t;
    }
    TILE_STAMP_SWEPT();
    const double* sd = ys[im];
    const double dui = LEAN ? ym : sd[g.self];
    double f[W - 1];
    if (have) {
        double pp = 0.0, pm = 0.0, umax = ui, umin = ui;
#pragma unroll
        for (int s = 0; s < W - 1; ++s) {
            const double uj = su[g.nb[s]];
            const double mij = mv[s], dij = dv[s];
            const double fs = mij * (dui - sd[g.nb[s]]) + dij * (ui - uj);
            f[s] = fs;
            pp += fmax(fs, 0.0);
            pm += fmin(fs, 0.0);
            const bool live = (mij != 0.0) || (dij != 0.0);
            umax = live ? fmax(umax, uj) : umax;
            umin = live ? fmin(umin, uj) : umin;
        }
        const double qp = umax - ui, qm = umin - ui;
        srp[g.self] = (pp != 0.0) ? fmin(1.0, mli * qp / (dt * pp)) : 1.0;
        srm[g.self] = (pm != 0.0) ? fmin(1.0, mli * qm / (dt * pm)) : 1.0;
    }
    __syncthreads();
    TILE_STAMP_FLUXES();
    if (g.owned) {
        const double rpi = srp[g.self], rmi = srm[g.self];
        double fbar = 0.0;
#pragma unroll
        for (int s = 0; s < W - 1; ++s) {
            const double fs = f[s];
            const double a = (fs > 0.0) ? fmin(rpi, srm[g.nb[s]]) : fmin(rmi, srp[g.nb[s]]);
            fbar += a * fs;
        }
        double* out = const_cast<double*>(vec_ptr(out_ref)) + bz * out_bstride;
        TILE_OUT(out[g.i], ui + dt * fbar / mli);
    }
    TILE_STAMP_END(3);
    step_end_by_last_workgroup(e);
}

// du/dt right-hand side + the first Chebyshev iterations in one launch (latency regime):
//   r = rhs - A u_L (helpers.py:1814), y_1 = w_1 r / Md, then iterations 2..K+1 (helpers.py:175-184).
// 12 x 12 tile + halo 10: one ring is spent on A u_L, nine on Chebyshev iterations 2..10.
// Also finalises the low-order solve's bookkeeping (what k_dudt_rhs does in the unfused sequence).
// GEOM: the off-diagonals of the mesh's own mass matrix from the cell geometry (as k_tile_cheb_flux_limit) instead of
// six loads per node.  PL (FEMFCT_TILE_FIT): patch edge 32 (12 x 12 tile) or 26 (6 x 6 tile, 11 waves: femfct_tile_fit).
// TRIM (FEMFCT_TILE_TRIM, lean loops): bit 1 -- the Jacobi launches left one partial per owning wave (part_count of them):
// all waves of the test's workgroup load them (deferred_test_load_wide); bit 8 -- write-through output stores (TILE_OUT).
// 0 is the kernel as it was.
template <int LEAN, int GEOM, int PL, int TRIM = 0>
__global__ void __launch_bounds__((PL * PL + WAVE - 1) / WAVE * WAVE)
k_tile_dudt_cheb(int n, int N, double h, MatRef A_ref, VecRef rhs_ref, int64_t rhs_bstride,
                 const double* __restrict__ M, const double* __restrict__ xa_, const double* __restrict__ xb_,
                 double* __restrict__ ulow_, double* __restrict__ rdu_, double* __restrict__ omid_,
                 double* __restrict__ oold_, double* __restrict__ part, StepCtl* __restrict__ ctl_, int budget,
                 int part_count, int iters_per_unit, double rel_tol, const double* __restrict__ partk, int exact_k,
                 int K, CheOmegas om, double md_scale, double omega1) {
    constexpr int W = 7, H = 10, PLD = PL + 1;
    constexpr bool CONE = LEAN == 2;
    static_assert(PL == TILE_L || LEAN, "fitted patches run the lean loops only");
    static_assert(!TRIM || LEAN == 1, "trimmed launches: lean loops");
    __shared__ double ys[LEAN ? 2 : 3][PL * PLD];
    __shared__ double smem[64];
    const int bz = blockIdx.z;
    StepCtl* ctl = ctl_ + bz;
    double* p = part + (int64_t)bz * 4 * FEMFCT_MAX_PARTIALS;
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    if (exact_k < 0 && blockIdx.y == gridDim.x) {
        // deferred test: the launch carries one extra row of workgroups; its first one does nothing but reduce the solve's
        // partials and write the step record (no tile behind it: no workgroup of the kernel ends later for it)
        if (blockIdx.x == 0) {
            const double* pk = partk + (int64_t)bz * 16 * FEMFCT_MAX_PARTIALS;
            if constexpr (TRIM & 1)
                deferred_test_publish(ctl, deferred_test_load_wide(p, pk, part_count, -exact_k, &ys[0][0]), -exact_k, iters_per_unit, rel_tol);
            else
                deferred_test_publish(ctl, deferred_test_load(p, pk, part_count, -exact_k), -exact_k, iters_per_unit, rel_tol);
        }
        return;
    }
    // deferred test (exact_k < 0): no launch of the solve set `done`, the iterate is the budget-parity one; nothing below
    // depends on the test's outcome, only the step log does -- workgroup 0 alone reduces the partials, requested here
    // and consumed after its own tile, so that nobody waits for them (nor for a look at the control block)
    const int parity = exact_k < 0 ? (budget & 1) : ctl->done ? ctl->parity : (budget & 1);
    if (exact_k >= 0)
        finalize_solve(ctl, p, part_count, budget, iters_per_unit, rel_tol, smem,
                       partk ? partk + (int64_t)bz * 16 * FEMFCT_MAX_PARTIALS : nullptr, exact_k, wg == 0);
    const int64_t voff = (int64_t)bz * n;
    const double* A = mat_ptr(A_ref, bz);
    const double* x = (parity ? xb_ : xa_) + voff;
    const double* rhs = vec_ptr(rhs_ref);
    if (rhs) rhs += bz * rhs_bstride;
    TILE_STAMP_BEGIN(H * PL + H);
    const TileGeom g = tile_geom<PL - 2 * H, H, PL>(N);
    double av[W], mv[W - 1], md = 1.0, rmd = 1.0, ui = 0.0, ri = 0.0;
#pragma unroll
    for (int s = 0; s < W; ++s) av[s] = 0.0;
#pragma unroll
    for (int s = 0; s < W - 1; ++s) mv[s] = 0.0;
    bool need_r = g.kvalid >= 1;            // r = rhs - A u_L on every node whose neighbours are in the patch
    if constexpr (CONE) {
        // r and y_1 only where an iterating node reads y_1 (d <= K): there the row of A, the rhs and the diagonal of M;
        // the off-diagonals of M where the node iterates at all (d < K); u_L one ring further out than r
        const int dist = tile_hexdist<H, PL>(g);
        need_r = need_r && dist <= K;
        if (g.inside && need_r) {
            md = M[g.i];
            rmd = 1.0 / (md_scale * md);
#pragma unroll
            for (int s = 0; s < W; ++s) av[s] = A[(int64_t)s * n + g.i];
            ri = rhs ? rhs[g.i] : 0.0;
        }
        if (g.inside && g.kvalid > 1 && dist < K) {
            if (GEOM) {
                const int pc = mass_edge_counts(g.gx, g.gy, N - 1);
                const double mq = (0.5 * h * h) / 12.0;
#pragma unroll
                for (int s = 1; s < W; ++s) mv[s - 1] = (double)((pc >> (2 * (s - 1))) & 3) * mq;
            } else {
#pragma unroll
                for (int s = 1; s < W; ++s) mv[s - 1] = M[(int64_t)s * n + g.i];
            }
        }
        if (g.inside && dist <= K + 1) ui = x[g.i];
    } else if (g.inside) {
        md = M[g.i];
        rmd = 1.0 / (md_scale * md);
#pragma unroll
        for (int s = 0; s < W; ++s) av[s] = A[(int64_t)s * n + g.i];
        if (GEOM) {
            const int pc = mass_edge_counts(g.gx, g.gy, N - 1);
            const double mq = (0.5 * h * h) / 12.0;
#pragma unroll
            for (int s = 1; s < W; ++s) mv[s - 1] = (double)((pc >> (2 * (s - 1))) & 3) * mq;
        } else {
#pragma unroll
            for (int s = 1; s < W; ++s) mv[s - 1] = M[(int64_t)s * n + g.i];
        }
        ui = x[g.i];
        ri = rhs ? rhs[g.i] : 0.0;
    }
    constexpr int UB = LEAN ? 0 : 2;        // the buffer u_L is staged in
    const bool spare = tile_spare<PL>();
    if (!spare) ys[UB][g.self] = ui;
    __syncthreads();
    TILE_STAMP_LOADED();
    double r = 0.0, y1 = 0.0;
    if (need_r) {
        double acc = av[0] * ui;
#pragma unroll
        for (int s = 1; s < W; ++s) acc = fma(av[s], ys[UB][g.nb[s - 1]], acc);
        r = -acc + ri;
        y1 = omega1 * (r / (md_scale * md));
    }
    if constexpr (LEAN) {
        // both buffers hold y_mid = y_1 (buffer 1 first: buffer 0 is still being read as u_L); y_mid and y_old of the
        // node itself stay in registers.  Iteration 0 reads buffer 1.
        if (!spare) ys[1][g.self] = y1;
        __syncthreads();
        if (!spare) ys[0][g.self] = y1;     // (own slot only, rewritten by this thread alone before anyone reads it)
        double ym = y1, yo = 0.0;
        const int dist = lean_dist<H, LEAN, PL>(g);
        const LeanAddr a = lean_addr<PL>(ys, g);
        auto live = [&](int k) { return k + 1 < g.kvalid && k < K - dist; };   // one ring already spent on A u_L
        int k = 0;
        for (; k + 1 < K; k += 2) {
            lean_cheb_iter<1, PL>(a, live(k), mv, md, rmd, r, om.w[k], ym, yo);
            lean_cheb_iter<0, PL>(a, live(k + 1), mv, md, rmd, r, om.w[k + 1], ym, yo);
        }
        if (k < K) lean_cheb_iter<1, PL>(a, live(k), mv, md, rmd, r, om.w[k], ym, yo);
        TILE_STAMP_SWEPT();
        if (g.owned) {
            TILE_OUT(ulow_[voff + g.i], ui);
            TILE_OUT(rdu_[voff + g.i], r);
            TILE_OUT(omid_[voff + g.i], ym);
            if (oold_) TILE_OUT(oold_[voff + g.i], yo);
        }
        TILE_STAMP_END(2);
        return;
    }
    __syncthreads();
    ys[0][g.self] = 0.0;
    ys[1][g.self] = y1;
    __syncthreads();
    int io = 0, im = 1, in_ = 2;
    for (int k = 0; k < K; ++k) {
        const double* ymd = ys[im];
        const double ymv = ymd[g.self];
        double yn = ymv;
        if (k + 1 < g.kvalid) {      // one ring already spent on A u_L
            double acc = md * ymv;
#pragma unroll
            for (int s = 0; s < W - 1; ++s) acc = fma(mv[s], ymd[g.nb[s]], acc);
            const double z = (r - acc) * rmd;
            const double yov = ys[io][g.self];
            yn = om.w[k] * (z + ymv - yov) + yov;
        }
        ys[in_][g.self] = yn;
        __syncthreads();
        int t = io; io = im; im = in_; in_ = t;
    }
    TILE_STAMP_SWEPT();
    if (g.owned) {
        ulow_[voff + g.i] = ui;
        rdu_[voff + g.i] = r;
        omid_[voff + g.i] = ys[im][g.self];
        if (oold_) oold_[voff + g.i] = ys[io][g.self];
    }
    TILE_STAMP_END(2);
}

}  // namespace

#ifdef FEMFCT_TUNING
// appends the phase sums since the last dump to `path` (one line per kernel) and clears them
void femfct_tile_phase_dump(const char* path) {
    static const char* names[4] = {"k_tile_build_jacobi", "k_tile_jacobi", "k_tile_dudt_cheb", "k_tile_cheb_flux_limit"};
    unsigned long long h[4][6];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tile_phase), sizeof(h)) != hipSuccess) return;
    if (FILE* f = fopen(path, "a")) {
        for (int k = 0; k < 4; ++k)
            if (h[k][2])
                fprintf(f, "%-24s launches %8llu  load phase %7.3f us  whole kernel %7.3f us  share %5.1f %%  after the last sweep %6.3f us"
                        "  (limiter: after the fluxes' barrier %6.3f us)\n", names[k], h[k][2], 0.01 * h[k][0] / h[k][2],
                        0.01 * h[k][1] / h[k][2], 100.0 * h[k][0] / (double)h[k][1], 0.01 * (h[k][1] - h[k][3]) / h[k][2],
                        k == 3 ? 0.01 * (h[k][1] - h[k][4]) / h[k][2] : 0.0);
        fclose(f);
    }
    memset(h, 0, sizeof(h));
    hipMemcpyToSymbol(HIP_SYMBOL(g_tile_phase), h, sizeof(h));
}
#endif

// ---- launchers, in the order of a step ---------------------------------------------------------------

// the LEAN template argument: 0 the loops as they were, 1 the lean loops, 2 the lean loops on the hexagonal cone
static int tile_lean_mode(const femfct_ctx* ctx) { return ctx->tile_lean ? (ctx->tile_cone ? 2 : 1) : 0; }

// ---- trimmed prologues and epilogues (FEMFCT_TILE_TRIM; the TRIM template argument of the four kernels) ----------------
// The bits of the knob that launches of this context may take at all: the variants exist for the plain lean loops.
static int tile_trim_mode(const femfct_ctx* ctx) { return tile_lean_mode(ctx) == 1 ? ctx->tile_trim & (TILE_TRIM_WAVES | TILE_TRIM_WT) : 0; }
int femfct_tile_trim_mask(const femfct_ctx* ctx) { return tile_trim_mode(ctx); }
static void tile_trim_count(femfct_ctx* ctx, int trim) {      // (flags, not counts: the launchers run for a context's lifetime)
    if (trim & TILE_TRIM_WAVES) ctx->trim_seen[0] = 1;
    if (trim & TILE_TRIM_WT) ctx->trim_seen[1] = 1;
}

// calls f with the mask (0, 1, 8 or 9) as a compile-time constant
template <class F>
static void with_trim(int trim, F&& f) {
    switch (trim) {
    case TILE_TRIM_WAVES: f(std::integral_constant<int, TILE_TRIM_WAVES>()); break;
    case TILE_TRIM_WT: f(std::integral_constant<int, TILE_TRIM_WT>()); break;
    case TILE_TRIM_WAVES | TILE_TRIM_WT: f(std::integral_constant<int, TILE_TRIM_WAVES | TILE_TRIM_WT>()); break;
    default: f(std::integral_constant<int, 0>()); break;
    }
}

// Bit 1: slots per array when the Jacobi launches of a deferred-test solve publish per owning wave; 0: per workgroup as
// before (knob off, other loops, or more slots than an array holds)
int femfct_tile_wave_slots(const femfct_ctx* ctx, const TilePlan& pl) {
    if (!(tile_trim_mode(ctx) & TILE_TRIM_WAVES)) return 0;
    const int64_t slots = (int64_t)pl.tiles * pl.tiles * tile_owning_waves(pl.H);
    return slots <= FEMFCT_MAX_PARTIALS ? (int)slots : 0;
}

// launch 0 with the operator construction fused in (latency regime; needs >= 2 launches in total because
// ||b|| is reduced by launch 1).  Later launches: femfct_enqueue_tile_jacobi(..., bn_launch = 1, g_build = tiles^2).
// pre: A is the pre-built L_k sequence (femfct_enqueue_low_seq; Nm must be null), D_k is not stored.
int femfct_enqueue_tile_build_jacobi(femfct_ctx* ctx, const TilePlan& pl, MatRef A, const double* Nm, int32_t nshared,
                                     VecRef rhs, int64_t rhs_bstride, VecRef u_n, int64_t u_bstride, double dt,
                                     int32_t batch, bool pre, bool wave_slots) {
    if (pre && Nm) return femfct_fail(ctx, FEMFCT_ERR_INVALID, "pre-built low-order operator with a non-flux matrix");
    const int trim = tile_trim_mode(ctx) & ((wave_slots ? TILE_TRIM_WAVES : 0) | TILE_TRIM_WT);
    tile_trim_count(ctx, trim);
    dim3 grid(pl.tiles, pl.tiles, batch);
    femfct_prof_begin(ctx, KC_JACOBI);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(STRIP_T), 0, ctx->stream, ctx->n, ctx->N, A, Nm, nshared, rhs, rhs_bstride, u_n,
                           u_bstride, ctx->d_ml, dt, ctx->d_L, ctx->d_D, ctx->d_b, ctx->d_xb, ctx->d_part, ctx->d_ctl, pl.K);
    };
    with_constant<8, TILE_HMAX>(pl.H, [&](auto h) {
        constexpr int H = decltype(h)::value;
        if (trim) {             // (lean loops without the cone: tile_trim_mode)
            with_trim(trim, [&](auto t) {
                constexpr int TRIM = decltype(t)::value;
                if (pre) go(k_tile_build_jacobi<H, 1, 1, TRIM>); else go(k_tile_build_jacobi<H, 0, 1, TRIM>);
            });
            return;
        }
        with_constant<0, 2>(tile_lean_mode(ctx), [&](auto l) {
            constexpr int LEAN = decltype(l)::value;
            if (pre) go(k_tile_build_jacobi<H, 1, LEAN>); else go(k_tile_build_jacobi<H, 0, LEAN>);
        });
    });
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

// L_k and D_k of `entries` consecutive sequence entries of A (k_low_seq); structured mesh in vertex order
int femfct_enqueue_low_seq(femfct_ctx* ctx, const double* A, double* L, double* D, int32_t entries, double dt) {
    if (!ctx->implicit_cols || ctx->W != 7 || (int64_t)ctx->N * ctx->N != ctx->n || entries < 1 || entries > 65535)
        return femfct_fail(ctx, FEMFCT_ERR_INVALID, "low-order sequence: structured mesh in vertex order only");
    femfct_prof_begin(ctx, KC_ASSEMBLE);
    hipLaunchKernelGGL(k_low_seq, dim3((ctx->n + 255) / 256, entries), dim3(256), 0, ctx->stream, ctx->n, ctx->N, A, ctx->d_ml,
                       dt, L, D);
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

int femfct_enqueue_tile_jacobi(femfct_ctx* ctx, const TilePlan& pl, const double* L, const double* b, double* xa,
                               double* xb, int launch, int g_build, int32_t batch, bool last, int bn_launch, int defer, bool wave_slots) {
    const bool big = femfct_tile_big(ctx, pl);
    // (the owning-wave epilogue belongs to deferred-test launches)
    const int trim = big ? 0 : tile_trim_mode(ctx) & (((wave_slots && defer) ? TILE_TRIM_WAVES : 0) | TILE_TRIM_WT);
    tile_trim_count(ctx, trim);
    double* bigp = big ? ctx->d_bigpart : nullptr;
    double* pk = ((last || defer) && !big) ? ctx->d_partk : nullptr;
    dim3 grid(pl.tiles, pl.tiles, batch);
    femfct_prof_begin(ctx, KC_JACOBI);
    auto go = [&](auto kernel, int defer_arg) {
        hipLaunchKernelGGL(kernel, grid, dim3(STRIP_T), 0, ctx->stream, ctx->n, ctx->N, L, b, xa, xb, ctx->d_part, ctx->d_ctl,
                           launch, pl.K, g_build, ctx->rel_tol, bigp, pk, bn_launch, defer_arg);
    };
    with_constant<0, 2>(tile_lean_mode(ctx), [&](auto l) {
        constexpr int LEAN = decltype(l)::value;
        if (big) {
            go(k_tile_jacobi<8, 0, 1, LEAN>, 0);
            femfct_launch_reduce_resid(ctx, (int64_t)pl.tiles * pl.tiles, launch, batch);
        } else {
            with_constant<8, TILE_HMAX>(pl.H, [&](auto h) {
                constexpr int H = decltype(h)::value;
                if constexpr (LEAN == 1) {
                    if (trim) {
                        with_trim(trim, [&](auto t) {
                            constexpr int TRIM = decltype(t)::value;
                            if constexpr (!(TRIM & TILE_TRIM_WAVES)) { if (pk && !defer) { go(k_tile_jacobi<H, 1, 0, 1, TRIM>, 0); return; } }
                            go(k_tile_jacobi<H, 0, 0, 1, TRIM>, defer);
                        });
                        return;
                    }
                }
                if (pk && !defer) go(k_tile_jacobi<H, 1, 0, LEAN>, 0); else go(k_tile_jacobi<H, 0, 0, LEAN>, defer);
            });
        }
    });
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

// the residual maximum of a launch on a grid with more workgroups than in-kernel partials (`count` per batch member);
// inside the caller's profiling bracket.  Also behind the 64-patch launches (kernels_patch64.hip).
void femfct_launch_reduce_resid(femfct_ctx* ctx, int64_t count, int launch, int32_t batch) {
    hipLaunchKernelGGL(k_reduce_resid, dim3(batch), dim3(STRIP_T), 0, ctx->stream, ctx->d_bigpart, count, ctx->d_ctl, launch);
}

// r, y_1 and Chebyshev iterations 2..(K+1) in one launch, the rest in ceil(.../10) tile launches.
// tail_first (optional): the caller runs the remaining iterations *tail_first .. iters itself (inputs
// mid = d_y0, old = d_y2), e.g. fused with the limiter; 0 is stored when nothing remains.
int femfct_enqueue_tile_dudt_cheb(femfct_ctx* ctx, MatRef A, VecRef rhs, int64_t rhs_bstride, double* ulow,
                                  int budget_units, int part_count, int iters_per_unit, int exact_k, int iters,
                                  const double* omegas, double md_scale, int32_t batch, int* tail_first, bool wave_slots) {
    constexpr int H = 10;
    const int trim = tile_trim_mode(ctx) & (((wave_slots && exact_k < 0) ? TILE_TRIM_WAVES : 0) | TILE_TRIM_WT);
    if (wave_slots && !(tile_trim_mode(ctx) & TILE_TRIM_WAVES))
        return femfct_fail(ctx, FEMFCT_ERR_INVALID, "per-wave partials outside the trimmed lean launches");
    tile_trim_count(ctx, trim);
    const int T = TILE_L - 2 * H, t = (ctx->N + T - 1) / T;
    const bool fit = femfct_tile_fit(ctx, batch);
    const int tl = fit ? (ctx->N + 5) / 6 : t;           // workgroups per side of this launch (the chained ones keep T = 12)
    const int K = std::min(iters - 1, H - 1);            // iterations 2..K+1 here
    CheOmegas om;
    for (int k = 0; k < K; ++k) om.w[k] = omegas[k + 1];
    const bool last = (K + 1 == iters);
    double* omid = last ? ctx->d_du : ctx->d_y0;
    double* oold = last ? nullptr : ctx->d_y2;
    femfct_prof_begin(ctx, KC_DUDT_RHS);
    auto go = [&](auto kernel, int PL) {
        hipLaunchKernelGGL(kernel, dim3(tl, exact_k < 0 ? tl + 1 : tl, batch), dim3((PL * PL + WAVE - 1) / WAVE * WAVE), 0,
                           ctx->stream, ctx->n, ctx->N, ctx->h, A, rhs, rhs_bstride, ctx->d_M, ctx->d_xa, ctx->d_xb, ulow, ctx->d_rdu,
                           omid, oold, ctx->d_part, ctx->d_ctl, budget_units, part_count, iters_per_unit, ctx->rel_tol,
                           exact_k ? ctx->d_partk : nullptr, exact_k, K, om, md_scale, omegas[0]);
    };
    // (the mass row from the geometry rides with the lean loops: FEMFCT_TILE_LEAN=0 is the kernel as it was)
    with_constant<0, 1>(ctx->tile_lean && femfct_geom_mass(ctx), [&](auto gm) {
        constexpr int GM = decltype(gm)::value;
        if (trim) {             // (lean loops without the cone: tile_trim_mode)
            with_trim(trim, [&](auto t) {
                constexpr int TRIM = decltype(t)::value;
                if (fit) go(k_tile_dudt_cheb<1, GM, 26, TRIM>, 26); else go(k_tile_dudt_cheb<1, GM, TILE_L, TRIM>, TILE_L);
            });
        } else if (fit) {
            if (ctx->tile_cone) go(k_tile_dudt_cheb<2, GM, 26>, 26); else go(k_tile_dudt_cheb<1, GM, 26>, 26);
        } else if constexpr (GM) {
            if (ctx->tile_cone) go(k_tile_dudt_cheb<2, 1, TILE_L>, TILE_L); else go(k_tile_dudt_cheb<1, 1, TILE_L>, TILE_L);
        } else {
            with_constant<0, 2>(tile_lean_mode(ctx), [&](auto l) { go(k_tile_dudt_cheb<decltype(l)::value, 0, TILE_L>, TILE_L); });
        }
    });
    femfct_prof_end(ctx);
    if (tail_first) *tail_first = last ? 0 : K + 2;
    if (last || tail_first) return FEMFCT_OK;
    TilePlan tp;
    tp.H = H; tp.K = H; tp.tiles = t;
    // remaining iterations K+2 .. iters; inputs (mid, old) = (y0, y2); scratch pair (y1, rp) then (y0, y2)
    return femfct_enqueue_tile_cheb(ctx, tp, ctx->d_rdu, ctx->d_y0, ctx->d_y2, ctx->d_du, K + 2, iters, omegas, md_scale,
                                    ctx->d_y1, ctx->d_rp, ctx->d_y0, ctx->d_y2, batch, nullptr);
}

int femfct_enqueue_tile_cheb(femfct_ctx* ctx, const TilePlan& pl, const double* b, const double* in_mid,
                             const double* in_old, double* y_out, int k_first, int k_last, const double* omegas,
                             double md_scale, double* bufA0, double* bufA1, double* bufB0, double* bufB1, int32_t batch,
                             const ChebIO* io_in) {
    ChebIO io0{};
    if (io_in) io0 = *io_in;
    io0.mid_ref = make_ref(nullptr); io0.mid_bs = 0; io0.out_ref = make_ref(nullptr); io0.out_bs = 0;
    for_cheb_launches(k_first, k_last, pl.K, omegas, in_mid, in_old, y_out, bufA0, bufA1, bufB0, bufB1,
                      [&](int k0, int k1, const CheOmegas& om, const double* mid, const double* old, double* omid, double* oold) {
        femfct_prof_begin(ctx, KC_CHEB);
        ChebIO io = io0;
        io.k0 = k0 - 1;
        if (io_in && k0 == k_first) { io.mid_ref = io_in->mid_ref; io.mid_bs = io_in->mid_bs; }
        if (io_in && k1 == k_last + 1) { io.out_ref = io_in->out_ref; io.out_bs = io_in->out_bs; }
        with_constant<8, TILE_HMAX>(pl.H, [&](auto h) {
            with_constant<0, 2>(tile_lean_mode(ctx), [&](auto l) {
                hipLaunchKernelGGL((k_tile_cheb<decltype(h)::value, decltype(l)::value>), dim3(pl.tiles, pl.tiles, batch),
                                   dim3(STRIP_T), 0, ctx->stream, ctx->n, ctx->N, ctx->d_M, b, mid, old, omid, oold, k1 - k0, om,
                                   md_scale, io);
            });
        });
        femfct_prof_end(ctx);
    });
    return FEMFCT_OK;
}

// what a limiter launch that also ends the step hands to step_end.h (level = null: the step end stays its own launch)
static EndArgs step_end_args(const femfct_ctx* ctx, int32_t batch, bool fuse_end) {
    EndArgs e{};
    e.level = nullptr;
    if (fuse_end) {
        e.level = ctx->d_level; e.delta = ctx->rep_last ? ctx->end_req_delta * ctx->rep_total : 0;
        e.ord_adv = ctx->rep_last ? ctx->rep_total : 0; e.ord_off = ctx->ord_bias; e.ctl = ctx->d_ctl; e.log = ctx->d_log;
        e.kctl = ctx->end_req_krylov ? (const KrylovCtl*)ctx->d_kry_ctl : nullptr; e.klog = (KrylovCtl*)ctx->d_klog;
        e.batch = batch; e.ticket = ctx->d_ticket;
    }
    return e;
}

int femfct_enqueue_tile_cheb_flux_limit(femfct_ctx* ctx, const double* b, const double* in_mid, const double* in_old,
                                        int k_first, int k_last, const double* omegas, double md_scale, MatRef D,
                                        const double* ulow, double dt, VecRef out, int64_t out_bstride, int32_t batch,
                                        bool fuse_end) {
    const int K = k_last - k_first + 1;
    if (K < 1 || K > 10) return femfct_fail(ctx, FEMFCT_ERR_INVALID, "fused Chebyshev tail: %d iterations", K);
    const EndArgs e = step_end_args(ctx, batch, fuse_end);
    CheOmegas om;
    for (int k = k_first; k <= k_last; ++k) om.w[k - k_first] = omegas[k - 1];
    const bool fit = femfct_tile_fit(ctx, batch);
    const int t = fit ? (ctx->N + 5) / 6 : (ctx->N + 7) / 8;
    const bool wt = (tile_trim_mode(ctx) & TILE_TRIM_WT) != 0;
    tile_trim_count(ctx, wt ? TILE_TRIM_WT : 0);
    femfct_prof_begin(ctx, KC_FLUX);
    auto go = [&](auto kernel, int PL) {
        hipLaunchKernelGGL(kernel, dim3(t, t, batch), dim3((PL * PL + WAVE - 1) / WAVE * WAVE), 0, ctx->stream, ctx->n, ctx->N,
                           ctx->h, ctx->d_M, b, in_mid, in_old, K, om, md_scale, D, ulow, ctx->d_ml, dt, out, out_bstride, e);
    };
    with_constant<0, 1>(femfct_geom_mass(ctx), [&](auto gm) {
        constexpr int GM = decltype(gm)::value;
        if (wt) {               // (lean loops without the cone: tile_trim_mode)
            if (fit) go(k_tile_cheb_flux_limit<GM, 1, 30, TILE_TRIM_WT>, 30);
            else go(k_tile_cheb_flux_limit<GM, 1, TILE_L, TILE_TRIM_WT>, TILE_L);
        } else if (fit) {
            if (ctx->tile_cone) go(k_tile_cheb_flux_limit<GM, 2, 30>, 30); else go(k_tile_cheb_flux_limit<GM, 1, 30>, 30);
        } else {
            with_constant<0, 2>(tile_lean_mode(ctx), [&](auto l) { go(k_tile_cheb_flux_limit<GM, decltype(l)::value, TILE_L>, TILE_L); });
        }
    });
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

// *fuse_end (in/out): whether this launch also does the step end (only the 16-patch variant can: see the kernel)
int femfct_enqueue_tile_flux_limit(femfct_ctx* ctx, const double* D, const double* ulow, const double* du, double dt,
                                   VecRef out, int64_t out_bstride, int32_t batch, bool* fuse_end_io, int half_d) {
    const bool fuse_end = fuse_end_io && *fuse_end_io && ctx->N <= 512;
    if (fuse_end_io) *fuse_end_io = fuse_end;
    const EndArgs e = step_end_args(ctx, batch, fuse_end);
    femfct_prof_begin(ctx, KC_FLUX);
    const bool geom = femfct_geom_mass(ctx);
    auto go = [&](auto kernel, int PL) {       // patch edge PL: tiles of PL - 2 FL_H nodes per side
        const int t = (ctx->N + PL - 2 * FL_H - 1) / (PL - 2 * FL_H);
        hipLaunchKernelGGL(kernel, dim3(t, t, batch), dim3(PL * PL), 0, ctx->stream, ctx->n, ctx->N, ctx->h, ctx->d_M, D, ulow, du,
                           ctx->d_ml, dt, out, out_bstride, e);
    };
    with_constant<0, 1>(geom, [&](auto g) {
        with_constant<0, 1>(half_d != 0, [&](auto hd) {
            constexpr int G = decltype(g)::value, HD = decltype(hd)::value;
            if (ctx->N <= 512) go(k_tile_flux_limit<16, G, HD>, 16); else go(k_tile_flux_limit<32, G, HD>, 32);
        });
    });
    femfct_prof_end(ctx);
    return FEMFCT_OK;
}

// ---- policy: which of the kernels above run, and how deep their halo is ------------------------------

// the registered mass matrix is the structured mesh's own and may be derived from the cell geometry (FEMFCT_GEOM_MASS)
bool femfct_geom_mass(const femfct_ctx* ctx) {
    return ctx->geom_mass && ctx->structured && ctx->mass_is_mesh && ctx->implicit_cols;
}

// one workgroup per CU is the regime where the fused tail pays (see femfct_tile_plan)
bool femfct_cheb_flux_fusable(const femfct_ctx* ctx, int32_t batch) {
    if (!ctx->fuse_flux || ctx->N > 512) return false;
    const int t = (ctx->N + 7) / 8;
    return (int64_t)t * t * batch <= ctx->wg_slots;
}

// Fitted patches of the fused du/dt and limiter launches (FEMFCT_TILE_FIT): 6 x 6 tiles, whose halos of 10 and 12 need
// patches of 26 and 30 nodes per side only (11 and 15 waves, a third fewer loads in the du/dt launch), while every
// workgroup -- the extra row of the deferred test included -- still gets a compute unit of its own.  Lean loops only.
bool femfct_tile_fit(const femfct_ctx* ctx, int32_t batch) {
    if (!ctx->tile_lean || !ctx->tile_fit) return false;
    const int t = (ctx->N + 5) / 6;
    return (int64_t)t * (t + 1) * batch <= ctx->wg_slots;
}

// The 32 x 32 patch is split as tile + 2 halos with halo H in {8, 9, 10}: H sweeps fit in one launch.
// Latency regime (small grids): pick the H that needs the fewest launches for the sweep budget
// (Chebyshev: 19 remaining iterations = 10 + 9 with H = 10).  Bandwidth regime (large grids): H = 8
// keeps the halo re-reading lowest.  need_partials: the Jacobi variant publishes one residual partial
// per workgroup, consumed in-kernel up to FEMFCT_MAX_PARTIALS workgroups (else a reduce kernel).
bool femfct_tile_plan(const femfct_ctx* ctx, TilePlan* pl, bool need_partials, int budget, int batch) {
    if (!femfct_tiles_usable(ctx)) return false;
    int H = 8;
    const bool small = ctx->N <= 512;
    if (small) {
        if (budget <= 0) H = 10;
        else {
            // fewest launches first, then the smallest halo.  Deep halos (11..13: tiles of 10..6 nodes per
            // side) only while every workgroup still gets its own CU -- there a launch costs ~4.4 us fixed
            // + ~0.3 us per sweep whatever the tile size (tools/lat_probe.hip), so 2 x 13 beats 3 x 9.
            int best = 1 << 30;
            for (int h = 8; h <= TILE_HMAX; ++h) {
                const int T = TILE_L - 2 * h, t = (ctx->N + T - 1) / T;
                if (h > 10 && (!ctx->deep_halo || (int64_t)t * t * batch > ctx->wg_slots)) break;
                int launches = (budget + h - 1) / h;
                if (launches < best) { best = launches; H = h; }
            }
        }
    }
    if (small && ctx->strip_k >= 8 && ctx->strip_k <= TILE_HMAX) H = ctx->strip_k;   // tuning knob (latency regime only)
    const int T = TILE_L - 2 * H;
    const int t = (ctx->N + T - 1) / T;
    if (need_partials && (int64_t)t * t > FEMFCT_MAX_PARTIALS) return false;
    if (t > 65535) return false;
    pl->tiles = t;
    pl->K = H;
    pl->H = H;
    return true;
}

bool femfct_tile_big(const femfct_ctx* ctx, const TilePlan& pl) {
    return (int64_t)pl.tiles * pl.tiles > FEMFCT_MAX_PARTIALS;
}

