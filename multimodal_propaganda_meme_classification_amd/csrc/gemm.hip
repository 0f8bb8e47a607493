// Grouped h16 MFMA GEMM with fused epilogue for gfx950 (see include/memehip.h): gemm_kernel below (128x128x64 tile, 8 waves, two
// workgroups per CU) in its three layouts -- forward (K-contiguous x K-contiguous), dgrad (x K-strided) and wgrad (K-strided x
// K-strided, f32 output + bias-gradient row sums) -- and gemm_skinny_kernel for forward / dgrad groups whose problems all have
// M <= 64 rows (one wave per 16 output columns, weights streamed to registers; same bits).  What follows describes gemm_kernel.
// Operands are staged by LDS-DMA (buffer_load ... lds: rows past the end of an operand read as zero, so M / the wgrad contraction
// need no padding), swizzle applied to the per-lane SOURCE address (gemm_tile.h):
//   K-contiguous operand tile  [128 rows][64 k]  (128-B rows): 16-B chunk c of row r lives at chunk c ^ (r & 7)
//                                                              -> ds_read_b128 fragments are conflict-free;
//   K-strided operand tile     [64 k][128 rows] (256-B rows): 32-B unit u of k-row k lives at unit u ^ ((k & 3) | ((k >> 3) & 1) << 2)
//                                                              -> ds_read_b64_tr_b16 fragments conflict-free.
// Epilogue: accumulators -> LDS as f32 [128][128] -> 16-B coalesced global stores with bias / GELU / gelu' / residual in f32.
// blockIdx -> tile: XCD-aware (blocks b, b+8 share an L2): each XCD gets a contiguous run of tiles, blocked for L2 (tile_coords).
#include "common.h"
#include "gemm_tile.h"

namespace {
using namespace mh_tile;

struct DevProblem {
    MhGemmProblem p;
    int tiles_n;
    int tile_start;
    int tiles_m;
    int kchunk;       // split-K (MhGemmProblem.ksplit > 1): contraction elements per split, a multiple of BK; 0 = no split
};
struct GemmGroup {
    int n;
    int total_tiles;
    int group_m;      // L2 blocking of the tile order: GROUP_M row panels are swept column by column (0/1: n-fastest)
    int pad_;
    unsigned long long* trace;   // debug (mh_gemm_set_trace): per workgroup 4 x 100-MHz stamps {entry, first stage landed, main loop done, stores issued}
    const int* rows_any;         // one of the problems' rows_dev pointers (NULL when no problem has one): a valid address for the unconditional loads of the live counts
    DevProblem d[MH_GEMM_MAX_GROUP];
};
MH_DEV void trace_stamp(const GemmGroup& g, int k) {
    if (g.trace && threadIdx.x == 0) g.trace[(size_t)blockIdx.x * 4 + k] = wall_clock64();
}

// ---- epilogue: f32 tile in LDS -> bias / GELU / gelu' / residual -> 16-B coalesced stores ----------
// The 16-bit epilogue operands (residual, gelu' pre-activation) are fetched BEFORE the accumulators go through
// LDS (epilogue_prefetch), so their HBM latency hides behind the LDS transpose + barrier instead of stalling
// every store iteration.
constexpr int EPI_THREADS = NW * 64;                  // the whole workgroup stores the BM x BN tile, 16 threads to a row
constexpr int EPI_ITERS = BM * 16 / EPI_THREADS;
struct EpiPrefetch {
    i32x4 res[EPI_ITERS], mul[EPI_ITERS];
};
MH_DEV void epilogue_prefetch(const MhGemmProblem& P, int m0, int n0, int tid, int M, EpiPrefetch& pf) {
#pragma unroll
    for (int it = 0; it < EPI_ITERS; ++it) {
        const int q = it * EPI_THREADS + tid;
        const int row = q >> 4, cc = q & 15;
        const int gm = min(m0 + row, M - 1), gn = min(n0 + cc * 8, P.N - 8);   // clamped: rows past M / columns past N are never stored
        const size_t o = (size_t)gm * P.ldc + gn;
        pf.res[it] = i32x4{0, 0, 0, 0};
        pf.mul[it] = i32x4{0, 0, 0, 0};
        if (P.residual) pf.res[it] = *(const i32x4*)((const h16*)P.residual + o);
        if (P.mul) pf.mul[it] = *(const i32x4*)((const h16*)P.mul + o);
    }
}

// ---- the per-element epilogue arithmetic: ONE pair of functions for gemm_kernel and gemm_skinny_kernel ----------
// Eight consecutive columns of one output row: v = alpha * acc + bias (epilogue_acc8) -> [dropout, in epilogue_rows] -> aux / activation
// (with the stored derivative) -> stored-derivative or gelu' multiply -> residual -> f32 (+=) or 16-bit store (epilogue_elem8).  Both
// kernels call them on the same f32 accumulator values, so a row computed by either is the same bits (tests/test_gemm_skinny_gpu.py);
// a copy would drift.  (The dropout step stays in epilogue_rows between the two: inside the shared function it cost gemm_kernel's
// dropout variant 8 spilled VGPRs.)
// (Everything it needs from the problem descriptor is copied to an EpiCtx of locals first: the descriptor lives in kernel-argument
//  memory, which the compiler must assume the stores alias, so it re-read every field after every store -- a chain of dependent
//  scalar loads per iteration.)
struct EpiCtx {
    int flags, ldc, N;
    float alpha;
    const h16* p_mul;
    const h16* p_res;
    h16* p_aux;
    void* p_c;
};
MH_DEV EpiCtx epi_ctx(const MhGemmProblem& P) {
    EpiCtx E;
    E.flags = P.flags;
    E.ldc = P.ldc;
    E.N = P.N;
    E.alpha = P.alpha == 0.f ? 1.0f : P.alpha;
    E.p_mul = (const h16*)P.mul;
    E.p_res = (const h16*)P.residual;
    E.p_aux = (h16*)P.aux;
    E.p_c = P.C;
    return E;
}
// epilogue_acc8: v = alpha * acc + bias for the eight accumulators x0 / x1 (b0 / b1: their bias, zeros without one).
MH_DEV void epilogue_acc8(const EpiCtx& E, const f32x4 x0, const f32x4 x1, const f32x4 b0, const f32x4 b1, float (&v)[8]) {
    const float alpha = E.alpha;
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = x0[e] * alpha + b0[e]; v[4 + e] = x1[e] * alpha + b1[e]; }
}
// epilogue_elem8: everything behind the dropout site (gemm_kernel's dropout variant applies its mask between the two; the skinny
// kernel never runs a problem with dropout).  (gm, gn): row and first column in the problem; pf_mul / pf_res: the 16-bit operands
// fetched ahead by the caller (zeros where the problem has none).
MH_DEV void epilogue_elem8(const EpiCtx& E, float (&v)[8], int gm, int gn, const i32x4 pf_mul, const i32x4 pf_res) {
    const int flags = E.flags;
    const h16* const p_mul = E.p_mul;
    const h16* const p_res = E.p_res;
    h16* const p_aux = E.p_aux;
    const size_t o = (size_t)gm * E.ldc + gn;
    if ((flags & MH_GEMM_GELU) && (flags & MH_GEMM_DERIV_AUX) && p_aux) {
        // activation and its derivative from the same exponential: aux receives act'(v), which the dgrad launch multiplies
        // by as it is (no transcendental math in the backward epilogue)
        Pack8 u;
        if (flags & MH_GEMM_QUICK_GELU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float sg = qgelu_sig(v[e]);
                u.e[e] = mh_f2bf(sg * (1.0f + 1.702f * v[e] * (1.0f - sg)));
                v[e] *= sg;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const GeluParts gp = gelu_parts(v[e]);
                u.e[e] = mh_f2bf(gp.cdf + v[e] * gp.pdf);
                v[e] *= gp.cdf;
            }
        }
        *(i32x4*)(p_aux + o) = u.v;
    } else {
        if (p_aux) {
            Pack8 u;
#pragma unroll
            for (int e = 0; e < 8; ++e) u.e[e] = mh_f2bf(v[e]);
            *(i32x4*)(p_aux + o) = u.v;
        }
        if (flags & MH_GEMM_GELU) {
            if (flags & MH_GEMM_QUICK_GELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = qgelu_f(v[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = gelu_f(v[e]);
            }
        }
    }
    if (p_mul) {
        Pack8 u;
        u.v = pf_mul;
        if (flags & MH_GEMM_DERIV_AUX) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= mh_bf2f(u.e[e]);
        } else if (flags & MH_GEMM_QUICK_GELU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= dqgelu_f(mh_bf2f(u.e[e]));
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= dgelu_f(mh_bf2f(u.e[e]));
        }
    }
    if (p_res) {
        Pack8 u;
        u.v = pf_res;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += mh_bf2f(u.e[e]);
    }
    if (flags & MH_GEMM_OUT_F32) {
        float* c = (float*)E.p_c + o;
        if (flags & MH_GEMM_ACCUM) {
            const f32x4 c0 = *(const f32x4*)c, c1 = *(const f32x4*)(c + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] += c0[e]; v[4 + e] += c1[e]; }
        }
        *(f32x4*)c = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)(c + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
        Pack8 u;
#pragma unroll
        for (int e = 0; e < 8; ++e) u.e[e] = mh_f2bf(v[e]);
        *(i32x4*)((h16*)E.p_c + o) = u.v;
    }
}

// (the bias -- a function of the thread's column only -- is loaded once: a per-iteration bias load sat behind the previous
//  iteration's store on the in-order vmcnt counter -- each iteration waited for a store to COMPLETE.)
template <bool DROP>
MH_DEV void epilogue_rows(const MhGemmProblem& P, const float* cs, int m0, int n0, int tid, int M, const EpiPrefetch& pf) {
    const EpiCtx E = epi_ctx(P);
    const int* const drop_rows = P.drop_rows;
    const DropCtx drop = mh_drop_ctx(DROP ? P.drop_rng : nullptr, P.drop_p, P.drop_stream);
    const int N = E.N;
    static_assert(EPI_THREADS % 16 == 0, "a thread keeps its column block across iterations");
    const int cc = tid & 15, gn = n0 + cc * 8;
    f32x4 b0 = f32x4{0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (P.bias && gn < N) {
        b0 = *(const f32x4*)(P.bias + gn);
        b1 = *(const f32x4*)(P.bias + gn + 4);
    }
    // ONE explicit wait for the bias / prefetched-operand loads, on every path, before the first iteration.  Without it each
    // iteration of the loop below began with a compiler-inserted s_waitcnt vmcnt(0): an iteration's body -- and the wait inside it --
    // is skipped when its row is past M, so at the next iteration's entry those loads are still pending on SOME path, and because
    // the other path has issued stores in between (loads and stores share the one in-order counter on gfx9) the only count the
    // compiler can prove is zero.  At run time that made iterations 2..4 wait for the previous iteration's global stores to
    // COMPLETE: three store round trips in every tile's epilogue (tools/isa_loadchain.py shows `S : b w0` per iteration before, none
    // after; round 4, second session).
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0), expcnt / lgkmcnt untouched
#pragma unroll
    for (int it = 0; it < EPI_ITERS; ++it) {
        const int row = (it * EPI_THREADS + tid) >> 4;
        const int gm = m0 + row;
        if (gm >= M || gn >= N) continue;      // ragged M; N need not fill the last 128-column tile (conv layers with 64 filters)
        const f32x4 x0 = *(const f32x4*)(cs + cs_index(row, cc * 8));
        const f32x4 x1 = *(const f32x4*)(cs + cs_index(row, cc * 8 + 4));
        float v[8];
        epilogue_acc8(E, x0, x1, b0, b1, v);
        if (DROP && drop.on) {     // nn.Dropout on the Linear output (BertSelfOutput / BertOutput), before the residual add
            const uint64_t dr = drop_rows ? (uint64_t)drop_rows[gm] : (uint64_t)gm;   // row in the unpacked tensor
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= mh_drop_mul(drop, dr * (uint64_t)N + (uint64_t)(gn + e));
        }
        epilogue_elem8(E, v, gm, gn, pf.mul[it], pf.res[it]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// gemm_kernel: the kernel of every grouped launch that gemm_skinny_kernel does not take.  128x128x64 tile per 512-thread workgroup: eight waves as
// 2 (M) x 4 (N), 64x32 each = 4x2 tiles of v_mfma_f32_16x16x32 (4 waves per SIMD cover barrier + LDS latency best on this path's
// shapes; 4 waves of 64x64 and 16 of 32x32 measured slower), two LDS-DMA stages, ONE barrier per K step, the next stage issued
// before the MFMAs of the current one.  Epilogue: accumulators -> f32 staging tile in LDS (swizzled: cs_index) -> bias / GELU /
// gelu' / residual in f32 -> 16-byte stores of whole 256-byte row segments; the 16-bit epilogue operands (residual, stored gelu')
// are fetched BEFORE the accumulators cross the LDS, so their latency hides behind the transpose.
// What limits it: per K step and CU the MFMA pipe (1 024 clocks for two resident workgroups), the LDS array
// (~1 280: 96 KB of fragment reads + 32 KB of LDS-DMA writes per workgroup) and the L2 -> LDS stream (1 024) are within 25 % of
// each other, and every launch pays ~4 us of fill + epilogue per round of 512 workgroups -- a burst of 16 MB of loads / stores
// that all workgroups issue at the same moment.
// Alternatives measured in the step against this kernel on one box (tools/lab/RESULTS.md (r4c) .. exp_r4g.sh;
// profiles/r04_gemm_shapes.csv; their source is in the history): the epilogue stored STRAIGHT from
// transposed accumulators (weights in the MFMA's A slot, v_permlane16_swap pairing, no staging tile) is 1-4 us faster on the
// store-only launches standalone and 3-5 us slower where a 16-bit operand is read back (64-byte row segments per wave instead of
// 256-byte ones) -- in the step: 9.75-9.84 ms against 9.66-9.72; the same kernel with 4 x 2 waves of 32x64 wins the weight-gradient
// launches by 5 % standalone and nothing in the step; the 128x256x32 tile loses 0.25 ms per step.
// ---------------------------------------------------------------------------------------------------------------------
template <int LA, int LB, bool DROP>
__global__ __launch_bounds__(512, 4) void gemm_kernel(const GemmGroup g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // ---- which tile ----------------------------------------------------------------------------
    trace_stamp(g, 0);
    // LIVE tiles (row layouts, LA == 0).  A problem over packed token rows (rows_dev) is laid out on the host for its MAXIMUM row
    // count; the row panels past the live count are tiles that only exit.  In the host's tile order they all sit at the END of the
    // list, i.e. in the last XCDs' contiguous runs: at 2 093 live of 4 096 text rows an N = 3072 launch gave XCD 7 nothing but dead
    // tiles and XCD 6 half of them -- the live work ran on 6.5 of the 8 XCDs.  The list is therefore re-counted here with the live row
    // panels only, and THAT list is cut into the eight XCD runs; the surplus workgroups (the highest block indices of every XCD,
    // dispatched last) exit.  Everything below is wave-uniform scalar arithmetic.
    int cnt[MH_GEMM_MAX_GROUP], tml[MH_GEMM_MAX_GROUP], liv[MH_GEMM_MAX_GROUP];
#pragma unroll
    for (int i = 0; i < MH_GEMM_MAX_GROUP; ++i) liv[i] = 0x7fffffff;
    if (LA == 0 && g.rows_any) {      // every problem's live count requested at once (a load behind `if (rows_dev)` is a dependent one)
        int v[MH_GEMM_MAX_GROUP];
#pragma unroll
        for (int i = 0; i < MH_GEMM_MAX_GROUP; ++i) {
            const int* src = (i < g.n && g.d[i].p.rows_dev) ? g.d[i].p.rows_dev : g.rows_any;
            v[i] = *src;
        }
#pragma unroll
        for (int i = 0; i < MH_GEMM_MAX_GROUP; ++i)
            if (i < g.n && g.d[i].p.rows_dev) liv[i] = __builtin_amdgcn_readfirstlane(v[i]);
    }
    int nwg = 0;
#pragma unroll
    for (int i = 0; i < MH_GEMM_MAX_GROUP; ++i) {
        cnt[i] = 0; tml[i] = 0;
        if (i < g.n) {
            tml[i] = g.d[i].tiles_m;
            cnt[i] = (i + 1 < g.n ? g.d[i + 1].tile_start : g.total_tiles) - g.d[i].tile_start;
            if (LA == 0 && g.d[i].p.rows_dev) {      // (never split-K: the host rejects rows_dev with ksplit)
                tml[i] = min(tml[i], (max(liv[i], 0) + BM - 1) / BM);
                cnt[i] = tml[i] * g.d[i].tiles_n;
            }
            nwg += cnt[i];
        }
    }
    int t;
    {
        const int b = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, x = b & 7, j = b >> 3;
        if (j >= q + (x < r ? 1 : 0)) return;      // beyond this XCD's run of live tiles
        t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    }
    int pi = 0, tstart = 0, tm_live = tml[0], live = liv[0];
    {
        int acc = 0;
#pragma unroll
        for (int i = 1; i < MH_GEMM_MAX_GROUP; ++i) {
            acc += cnt[i - 1];
            if (i < g.n && t >= acc) { pi = i; tstart = acc; tm_live = tml[i]; live = liv[i]; }
        }
    }
    const MhGemmProblem& P = g.d[pi].p;
    int lt = t - tstart;
    // split-K: the problem's tiles are replicated ksplit times; split s contracts over [s * kchunk, (s+1) * kchunk) and
    // writes its own f32 partial output at C + s * M * ldc (summed by the caller: mh_colsum_partials_f32)
    const int kchunk = g.d[pi].kchunk;
    int ksplit_idx = 0;
    if (kchunk > 0) {
        const int per = g.d[pi].tiles_m * g.d[pi].tiles_n;
        ksplit_idx = lt / per;
        lt -= ksplit_idx * per;
    }
    int tm, tn;
    tile_coords(g.d[pi].tiles_n, tm_live, g.group_m, lt, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    int M = P.M, K = P.K;
    const int N = P.N;
    if (P.rows_dev) {   // packed (padding-free) token rows: the live row count is only known on the device
        if (LA == 0) {
            M = min(M, live);
            if (m0 >= M) return;     // (cannot happen for live tiles; kept as the bound of the partial last panel)
        } else {
            K = min(K, __builtin_amdgcn_readfirstlane(*P.rows_dev));      // (uniform: a VGPR here puts the operand's buffer resource in VGPRs and a waterfall loop around every LDS-DMA load)
        }
    }
    const int kbeg = ksplit_idx * kchunk;                       // 0 without split-K
    const int kend = kchunk > 0 ? min(K, kbeg + kchunk) : K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const uint32_t a_bytes = (LA == 0) ? (uint32_t)((M - 1) * P.lda + K) * 2u
                                       : (uint32_t)((K - 1) * P.lda + M) * 2u;
    const uint32_t b_bytes = (LB == 0) ? (uint32_t)((N - 1) * P.ldb + K) * 2u
                                       : (uint32_t)((K - 1) * P.ldb + N) * 2u;
    const __amdgpu_buffer_rsrc_t ra = mh_rsrc(P.A, a_bytes);
    const __amdgpu_buffer_rsrc_t rb = mh_rsrc(P.B, b_bytes);

    // weight gradient: the bias gradient = row sums of A, one more MFMA per A fragment against ones (column tile 0, waves of column 0)
    f32x4 accb[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_rowsum = (LA == 1) && (P.rowsum != nullptr) && (tn == 0) && ((wave % NWN) == 0);
    h16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (h16)1.0f;

    const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
    // (static s_setprio(1) for waves 4-7 -- the younger half of the workgroup, MI355X_MICROARCH.md "two waves per SIMD" item 4 -- measured:
    //  10.12-10.18 ms per step against 10.09-10.11, same box, three alternations: nothing)
    f32x4 acc[NI][NJ];
    // (SCOPED = true: without it the K-strided fragment reads drained the next stage's DMA at the top of every K step, gemm_tile.h)
    k_loop<LA, LB, true>(
        acc, smem, nk, wave, lane,
        [&](int kt, char* st) {
            dma_tile<LA>(ra, P.lda, m0, kbeg + kt * BK, wave, lane, st);
            dma_tile<LB>(rb, P.ldb, n0, kbeg + kt * BK, wave, lane, st + BM * BK * 2);
        },
        [&](const h16x8 (&fa)[NI]) {
            if (do_rowsum) {
#pragma unroll
                for (int i = 0; i < NI; ++i) accb[i] = MH_MFMA_16x16x32(fa[i], ones, accb[i], 0, 0, 0);
            }
        },
        [&] { trace_stamp(g, 1); });

    // ---- epilogue --------------------------------------------------------------------------------
    trace_stamp(g, 2);
    if (do_rowsum && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wave_m0(wave) + i * 16 + (lane >> 4) * 4 + r;
                if (row < M) P.rowsum[row] = accb[i][r] * (P.alpha == 0.f ? 1.0f : P.alpha);
            }
    }
    float* cs = (float*)smem;  // [128][128] f32 staging tile
    if (kchunk > 0) {       // split-K partial: plain f32 store of alpha * acc into this split's slab, no epilogue operands
        stage_acc(cs, acc, wave, lane);
        __syncthreads();
        float* slab = (float*)P.C + (size_t)ksplit_idx * (size_t)P.M * (size_t)P.ldc;
        store_slab(slab, cs, P.alpha == 0.f ? 1.0f : P.alpha, m0, n0, M, N, P.ldc, tid);
        trace_stamp(g, 3);
        return;
    }
    // (issuing these loads under the last K tile's MFMAs instead was measured 20 % slower: the extra live registers
    //  across the main loop cost more than the remaining exposed latency)
    EpiPrefetch pf;
    epilogue_prefetch(P, m0, n0, tid, M, pf);
    stage_acc(cs, acc, wave, lane);
    __syncthreads();
    epilogue_rows<DROP>(P, cs, m0, n0, tid, M, pf);
    trace_stamp(g, 3);
}

// ---------------------------------------------------------------------------------------------------------------------
// gemm_skinny_kernel: grouped launches whose problems ALL have M <= 64 rows (the compact last encoder layer: [B, D] panels; the
// caption decoder's step), layouts forward (0,0) and dgrad (0,1).  gemm_kernel gives such a launch N / 128 workgroups -- 6 to 48
// of them on 256 CUs -- each walking its K tiles one memory round trip at a time.  Here ONE WAVE is a workgroup and owns SKN_BN = 16
// output columns and all the rows: N / 16 workgroups per problem, and the weight fragment of v_mfma_f32_16x16x32 -- 16 contiguous
// bytes per lane in the forward layout -- goes straight from memory to VGPRs, D K tiles ahead: a register ring the compiler waits on
// with counted vmcnt (the ring's turns hold no branch, and every load is unconditional; past the last K tile its offset is outside
// the buffer, which reads as zero without a memory access).  No LDS, no barrier in the forward K loop.  The K-strided weights of the
// dgrad layout come as 32-byte row pieces through the same ring, are written to a wave-private [64 k][16] LDS image when their tile
// is due and read back with ds_read_b64_tr_b16 (the addressing of gemm_tile.h: read_frag<1>); LDS operations of one wave execute in
// order, so no barrier there either.
// The [M, K] activation panel is read by every workgroup (L2-resident): both 32-deep halves of a row's K tile = one 128-byte line.
// Same bits as gemm_kernel: the same MFMA with A rows / B columns in the same lanes and the same k in the same fragment element, one
// f32 accumulator per output element, K tiles ascending with their two halves in order, and epilogue_acc8 / epilogue_elem8 on it.
// MI = 16-row blocks (2: M <= 32, 4: M <= 64); D = K tiles in flight (skn_depth: 8 / 4, i.e. ~48 / ~40 KB per wave).
// Widths and depths that were measured against these: profiles/r16_skinny_gemm.txt.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SKN_NJ = 1;                 // 16-column blocks per wave
constexpr int SKN_BN = 16 * SKN_NJ;
constexpr int SKN_MAX_M = 64;
constexpr int SKN_CS_LD = SKN_BN + 4;     // f32 staging rows + 4 pad: the four 16-lane groups of an accumulator store hit four bank quarters
constexpr uint32_t SKN_PAST_END = 0x80000000u;      // a byte offset beyond every buffer this kernel binds (operands are < 2 GiB)
constexpr int skn_depth(int mi) { return mi <= 2 ? 8 : 4; }

template <int MI>
struct SknFrag {
    i32x4 a[MI][2], b[SKN_NJ * 2];      // forward: b[j * 2 + kk]; dgrad: piece p = k rows p * (32 / NJ) ..
};

template <int LB, int MI>
__global__ __launch_bounds__(64) void gemm_skinny_kernel(const GemmGroup g) {
    constexpr int D = skn_depth(MI), NJ = SKN_NJ, CPR = 2 * NJ;      // CPR: 16-byte chunks per row of BN columns
    constexpr int CS_FLOATS = MI * 16 * SKN_CS_LD, IMG_FLOATS = BK * SKN_BN * 2 / 4;      // dgrad: the [64 k][BN] weight image first
    __shared__ __attribute__((aligned(16))) float cs[CS_FLOATS > IMG_FLOATS ? CS_FLOATS : IMG_FLOATS];
    int t;
    {      // XCD-aware as in gemm_kernel: each XCD gets a contiguous run of column tiles (neighbours share weight lines in its L2)
        const int nwg = g.total_tiles, b = blockIdx.x;
        const int q = nwg >> 3, r = nwg & 7, x = b & 7, j = b >> 3;
        if (j >= q + (x < r ? 1 : 0)) return;
        t = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    }
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MH_GEMM_MAX_GROUP; ++i)
        if (i < g.n && t >= g.d[i].tile_start) pi = i;
    const MhGemmProblem& P = g.d[pi].p;
    const int n0 = (t - g.d[pi].tile_start) * SKN_BN;
    const int M = P.M, N = P.N, K = P.K, lda = P.lda, ldb = P.ldb;
    const int lane = threadIdx.x, r16 = lane & 15, g4 = lane >> 4;
    const __amdgpu_buffer_rsrc_t ra = mh_rsrc(P.A, (uint32_t)((M - 1) * lda + K) * 2u);
    const __amdgpu_buffer_rsrc_t rb = mh_rsrc(P.B, LB == 0 ? (uint32_t)((N - 1) * ldb + K) * 2u : (uint32_t)((K - 1) * ldb + N) * 2u);
    const int nk = K / BK;

    // per-lane byte offsets of K tile 0.  A block i: row i * 16 + r16, k = kk * 32 + g4 * 8 (rows >= M lie past the buffer: zeros).
    // B forward: column n0 + j * 16 + r16 at the same k; B dgrad: piece p = k rows p * (64 / CPR) + lane / CPR, columns
    // n0 + (lane % CPR) * 8 .. + 7 (columns >= N: zeros or a neighbour's values, feeding only output columns that are never stored).
    const uint32_t a_off = (uint32_t)(r16 * lda + g4 * 8) * 2u, a_blk = (uint32_t)(16 * lda) * 2u;
    const uint32_t b_off = LB == 0 ? (uint32_t)((n0 + r16) * ldb + g4 * 8) * 2u : (uint32_t)((lane / CPR) * ldb + n0 + (lane % CPR) * 8) * 2u;
    const uint32_t b_blk = (uint32_t)(16 * ldb) * 2u;                 // forward: the next 16 columns
    const uint32_t b_piece = (uint32_t)((64 / CPR) * ldb) * 2u;       // dgrad: the next 64 / CPR k rows
    const uint32_t b_tile = LB == 0 ? (uint32_t)BK * 2u : (uint32_t)(BK * ldb) * 2u;
    auto load = [&](SknFrag<MI>& f, int kt) {
        const bool in = kt < nk;
        const uint32_t ao = in ? a_off + (uint32_t)kt * (BK * 2u) : SKN_PAST_END;
        const uint32_t bo = in ? b_off + (uint32_t)kt * b_tile : SKN_PAST_END;
#pragma unroll
        for (int p = 0; p < CPR; ++p) f.b[p] = mh_buf_load16(rb, LB == 0 ? bo + (p >> 1) * b_blk + (p & 1) * 64u : bo + p * b_piece);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) f.a[i][h] = mh_buf_load16(ra, ao + i * a_blk + h * 64u);
    };

    f32x4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    SknFrag<MI> ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load(ring[s], s);
    char* const wimg = (char*)cs;
    auto consume = [&](const SknFrag<MI>& f) {
        Pack8 fb[NJ][2];
        if (LB == 0) {
#pragma unroll
            for (int p = 0; p < CPR; ++p) fb[p >> 1][p & 1].v = f.b[p];
        } else {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int p = 0; p < CPR; ++p) *(i32x4*)(wimg + p * 1024 + lane * 16) = f.b[p];      // rows of BN * 2 bytes, linear
            asm volatile("" ::: "memory");
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int k0 = kk * 32 + g4 * 8 + (r16 >> 2);      // lanes 4q..4q+3 supply k row k0 (and k0 + 4), 8 bytes each
                    const int at = k0 * (SKN_BN * 2) + j * 32 + (r16 & 3) * 8;
                    union {
                        struct { s16x4 lo, hi; } s;
                        h16x8 h;
                    } cv;
                    cv.s.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, wimg + at));
                    cv.s.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, wimg + at + 4 * (SKN_BN * 2)));
                    fb[j][kk].h = cv.h;
                }
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                Pack8 fa;
                fa.v = f.a[i][kk];
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = MH_MFMA_16x16x32(fa.h, fb[j][kk].h, acc[i][j], 0, 0, 0);
            }
    };
    // whole turns of the ring: no branch between the loads, so every wait is a counted one ((D - 1) tiles stay in flight) ...
    int kt0 = 0;
    for (; kt0 + D <= nk; kt0 += D) {
#pragma unroll
        for (int s = 0; s < D; ++s) {
            consume(ring[s]);
            load(ring[s], kt0 + s + D);
        }
    }
    // ... and the last nk % D tiles, already in the ring
    const int rem = nk - kt0;
#pragma unroll
    for (int s = 0; s < D - 1; ++s)
        if (s < rem) consume(ring[s]);      // (uniform)

    // ---- epilogue: accumulators -> wave-private f32 image -> 8 columns of a row per lane -> the shared epilogue arithmetic ----
    const EpiCtx E = epi_ctx(P);
    constexpr int iters = MI * 16 * CPR / 64, RPI = 64 / CPR;      // rows per iteration
    const int cc = lane % CPR, gn = n0 + cc * 8;
    f32x4 b0 = f32x4{0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (P.bias && gn < N) {
        b0 = *(const f32x4*)(P.bias + gn);
        b1 = *(const f32x4*)(P.bias + gn + 4);
    }
    i32x4 pf_mul[iters], pf_res[iters];
#pragma unroll
    for (int it = 0; it < iters; ++it) {      // (clamped: rows past M / columns past N are never stored)
        const size_t o = (size_t)min(it * RPI + lane / CPR, M - 1) * E.ldc + min(gn, N - 8);
        pf_mul[it] = pf_res[it] = i32x4{0, 0, 0, 0};
        if (E.p_res) pf_res[it] = *(const i32x4*)(E.p_res + o);
        if (E.p_mul) pf_mul[it] = *(const i32x4*)(E.p_mul + o);
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) cs[(i * 16 + g4 * 4 + r) * SKN_CS_LD + j * 16 + r16] = acc[i][j][r];
    asm volatile("" ::: "memory");
#pragma unroll
    for (int it = 0; it < iters; ++it) {
        const int gm = it * RPI + lane / CPR;
        if (gm >= M || gn >= N) continue;
        const f32x4 x0 = *(const f32x4*)(cs + gm * SKN_CS_LD + cc * 8);
        const f32x4 x1 = *(const f32x4*)(cs + gm * SKN_CS_LD + cc * 8 + 4);
        float v[8];
        epilogue_acc8(E, x0, x1, b0, b1, v);
        epilogue_elem8(E, v, gm, gn, pf_mul[it], pf_res[it]);
    }
}

// The dispatch rule of mh_gemm_bf16_grouped, from the problem list alone (mh_gemm_skinny_eligible exports it)
// Width bound: a launch that gives gemm_kernel 128 or more column tiles (half the CUs and up) streams its weights as fast there, and
// every 16-column wave here re-reads the whole activation panel: at M = 64, K = 768 the skinny kernel wins x2.1 at N = 4096, x1.2 at
// 12288, ties at 16384 (128 tiles) and loses x0.75 at 24576 and x0.67 on the decoder's logits, N = 30528 (profiles/r16_skinny_gemm.txt).
constexpr int SKN_WIDE_TILES = 128;
bool skinny_eligible(const MhGemmProblem* problems, int n, int a_kmajor, int b_kmajor) {
    if (!problems || n < 1 || n > MH_GEMM_MAX_GROUP || a_kmajor) return false;
    int wide_tiles = 0;
    for (int i = 0; i < n; ++i) {
        const MhGemmProblem& p = problems[i];
        if (p.M < 1 || p.M > SKN_MAX_M || p.rows_dev || p.ksplit > 1 || p.drop_rng) return false;
        wide_tiles += (p.N + BN - 1) / BN;
    }
    return wide_tiles < SKN_WIDE_TILES;
}

template <int LB, int MI>
int launch_skinny2(const GemmGroup& g, hipStream_t s) {
    hipLaunchKernelGGL((gemm_skinny_kernel<LB, MI>), dim3(g.total_tiles), dim3(64), 0, s, g);
    return mh_launch_status();
}
// (the problems were validated by the caller)
int launch_skinny(GemmGroup& g, int b_kmajor, hipStream_t s) {
    int total = 0, max_m = 0;
    for (int i = 0; i < g.n; ++i) {
        g.d[i].tiles_n = (g.d[i].p.N + SKN_BN - 1) / SKN_BN;
        g.d[i].tiles_m = 1;
        g.d[i].tile_start = total;
        total += g.d[i].tiles_n;
        max_m = g.d[i].p.M > max_m ? g.d[i].p.M : max_m;
    }
    g.total_tiles = total;
    if (max_m <= 32) return b_kmajor ? launch_skinny2<1, 2>(g, s) : launch_skinny2<0, 2>(g, s);
    return b_kmajor ? launch_skinny2<1, 4>(g, s) : launch_skinny2<0, 4>(g, s);
}

unsigned long long* g_trace = nullptr;      // mh_gemm_set_trace

template <int LA, int LB, bool DROP>
int launch2(const GemmGroup& g, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)gemm_kernel<LA, LB, DROP>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_kernel<LA, LB, DROP>), dim3(g.total_tiles), dim3(512), LDS_BYTES, s, g);
    return mh_launch_status();
}
template <int LA, int LB>
int launch(const GemmGroup& g, hipStream_t s) {
    if constexpr (LA == 0 && LB == 0) {     // the dropout epilogue is compiled only for the layout that runs it (forward), in a kernel of its own
        bool any_drop = false;
        for (int i = 0; i < g.n; ++i) any_drop |= (g.d[i].p.drop_rng != nullptr && g.d[i].p.drop_p > 0.f);
        if (any_drop) return launch2<LA, LB, true>(g, s);
    }
    return launch2<LA, LB, false>(g, s);
}

}  // namespace

extern "C" int mh_gemm_bf16_grouped(const MhGemmProblem* problems, int n_problems, int a_kmajor,
                                    int b_kmajor, mh_stream_t stream) {
    if (!problems || n_problems < 1 || n_problems > MH_GEMM_MAX_GROUP) return MH_EINVAL;
    GemmGroup g;
    g.n = n_problems;
    int total = 0;
    for (int i = 0; i < n_problems; ++i) {
        const MhGemmProblem& p = problems[i];
        if (!p.A || !p.B || !p.C) return MH_EINVAL;
        if (p.M < 1 || p.N < 1 || p.K < 1) return MH_ESHAPE;
        if (p.N % 8) return MH_ESHAPE;
        if (a_kmajor && (p.M % 8)) return MH_ESHAPE;
        if (!(a_kmajor && b_kmajor) && (p.K % BK)) return MH_ESHAPE;
        if ((p.lda % 8) || (p.ldb % 8) || (p.ldc % 8)) return MH_ESHAPE;
        if (((uintptr_t)p.A | (uintptr_t)p.B | (uintptr_t)p.C) & 15) return MH_EINVAL;
        if (p.rowsum && !a_kmajor) return MH_EINVAL;
        if ((p.flags & MH_GEMM_ACCUM) && !(p.flags & MH_GEMM_OUT_F32)) return MH_EINVAL;
        g.d[i].p = p;
        g.d[i].tiles_n = (p.N + BN - 1) / BN;
        g.d[i].tile_start = total;
        g.d[i].tiles_m = (p.M + BM - 1) / BM;
        g.d[i].kchunk = 0;
        int splits = 1;
        if (p.ksplit > 1) {       // split-K: f32 output slabs [ksplit][M][ldc], no fused epilogue
            if (!(p.flags & MH_GEMM_OUT_F32) || (p.flags & (MH_GEMM_ACCUM | MH_GEMM_GELU)) || p.bias || p.residual || p.aux || p.mul ||
                p.rowsum || p.rows_dev || p.drop_rng)
                return MH_EINVAL;
            const int kc = ksplit_chunk(p.K, p.ksplit);
            g.d[i].kchunk = kc;
            splits = (p.K + kc - 1) / kc;          // splits that actually hold rows (<= ksplit); the caller zero-fills the rest
            if (splits != p.ksplit) return MH_ESHAPE;
        }
        total += g.d[i].tiles_m * g.d[i].tiles_n * splits;
    }
    g.total_tiles = total;
    g.group_m = GROUP_M;
    g.pad_ = 0;
    g.trace = g_trace;
    g.rows_any = nullptr;
    for (int i = 0; i < n_problems; ++i)
        if (problems[i].rows_dev && !g.rows_any) g.rows_any = problems[i].rows_dev;
    hipStream_t s = (hipStream_t)stream;
    if (skinny_eligible(problems, n_problems, a_kmajor, b_kmajor)) return launch_skinny(g, b_kmajor, s);
    if (!a_kmajor && !b_kmajor) return launch<0, 0>(g, s);
    if (!a_kmajor && b_kmajor) return launch<0, 1>(g, s);
    if (a_kmajor && b_kmajor) return launch<1, 1>(g, s);
    return MH_EINVAL;  // (1,0) is not needed by the path
}

extern "C" int mh_gemm_ksplit_for(int K, int want) { return ksplit_fit(K, want); }

extern "C" int mh_gemm_skinny_eligible(const MhGemmProblem* problems, int n_problems, int a_kmajor, int b_kmajor) {
    return skinny_eligible(problems, n_problems, a_kmajor, b_kmajor) ? 1 : 0;
}

// profiling knob: with a device buffer of 4 x 8 bytes per workgroup of the largest launch, the kernel records 100-MHz stamps per
// workgroup {entry, first K stage landed, main loop done, epilogue stores issued}; NULL switches it off (tools/gemm_timeline.py)
extern "C" int mh_gemm_set_trace(void* device_buffer) {
    g_trace = (unsigned long long*)device_buffer;
    return MH_OK;
}
