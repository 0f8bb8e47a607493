// The MFMA tile core shared by the GEMM (gemm.hip: gemm_kernel) and the implicit-GEMM convolution (convgemm.hip:
// conv_gemm_kernel): 128x128x64 tiles, eight waves, swizzled [rows][64 k] / [64 k][rows] LDS images filled by LDS-DMA, MFMA
// fragment reads, the GROUP_M tile order, the two-stage K loop, the f32 staging tile and the split-K slab store.  Both kernels run
// the same K loop, so a convolution and the GEMM over its explicit im2col matrix give the same bits.  What stays in each kernel:
// its XCD distribution of the tiles, how a K stage is issued, and its epilogue.
#pragma once
#include "common.h"

namespace mh_tile {

constexpr int BM = 128, BN = 128, BK = 64;
// eight waves as 2 (M) x 4 (N), 64x32 each = NI x NJ = 4 x 2 tiles of v_mfma_f32_16x16x32
constexpr int NW = 8, NWM = 2, NWN = 4, NI = BM / NWM / 16, NJ = BN / NWN / 16;
MH_DEV int wave_m0(int wave) { return (wave / NWN) * (NI * 16); }      // first row / column of the wave's 64x32 block
MH_DEV int wave_n0(int wave) { return (wave % NWN) * (NJ * 16); }
constexpr int STAGE_BYTES = (BM * BK + BN * BK) * 2;  // 32 KiB
constexpr int LDS_BYTES = 2 * STAGE_BYTES;            // 64 KiB

MH_DEV int swz_kstrided(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }

// ---- global -> LDS directly (LDS-DMA, buffer_load ... lds): no VGPR staging, no ds_write pass ---
// One wave-instruction writes 1 KiB of LDS linearly (base + lane*16), so the swizzle is applied to
// the per-lane SOURCE address (an involution: read_frag applies the same one).  A tile is 16 such pieces: wave w moves 2w and 2w+1.
constexpr int DMA_PPW = 16 / NW;
template <int KMAJOR>
MH_DEV void dma_tile(__amdgpu_buffer_rsrc_t r, int ld, int r0, int k0, int wave, int lane, char* lds) {
#pragma unroll
    for (int i = 0; i < DMA_PPW; ++i) {
        const int piece = wave * DMA_PPW + i;
        uint32_t off;
        if (KMAJOR == 0) {
            const int row = piece * 8 + (lane >> 3);
            const int c = (lane & 7) ^ (row & 7);
            off = (uint32_t)((r0 + row) * ld + k0 + c * 8) * 2u;
        } else {
            const int kr = piece * 4 + (lane >> 4);
            const int pos = lane & 15;
            const int c = (((pos >> 1) ^ swz_kstrided(kr)) << 1) | (pos & 1);
            off = (uint32_t)((k0 + kr) * ld + r0 + c * 8) * 2u;
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, LDS_PTR(void, lds + piece * 1024), 16, off, 0, 0, 0);
    }
}

// ---- LDS -> MFMA fragment: rows rb..rb+15, k = kk*32 .. kk*32+31 -------------------------------
template <int KMAJOR>
MH_DEV h16x8 read_frag(const char* lds, int rb, int kk, int lane) {
    if (KMAJOR == 0) {
        const int row = rb + (lane & 15);
        const int c = kk * 4 + (lane >> 4);
        Pack8 u;
        u.v = *(const i32x4*)(lds + row * 128 + ((c ^ (row & 7)) << 4));
        return u.h;
    } else {
        const int i = lane & 15, g = lane >> 4;
        const int q = i >> 2, p = i & 3;
        const int k0 = kk * 32 + g * 8 + q;  // first block row supplied by this lane
        const int u = rb >> 4;               // 32-B unit of the 16 columns
        const int inner = ((p >> 1) << 4) | ((p & 1) << 3);
        const int a0 = k0 * 256 + ((u ^ swz_kstrided(k0)) << 5) + inner;
        const int k1 = k0 + 4;
        const int a1 = k1 * 256 + ((u ^ swz_kstrided(k1)) << 5) + inner;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, lds + a0));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, lds + a1));
        union {
            struct { s16x4 lo, hi; } s;
            h16x8 h;
        } cv;
        cv.s.lo = lo;
        cv.s.hi = hi;
        return cv.h;
    }
}

// The same read with an alias scope on it.  While an LDS-DMA is pending, hipcc puts `s_waitcnt vmcnt(0)` in front of every LDS read that
// carries no alias information: the plain ds_read_b128 loads carry their type's, the ds_read_tr16_b64 builtin carries none.  In k_loop
// the DMA of K tile kt + 1 is issued at the top of step kt, so the K-strided fragment reads of tile kt waited for it to land -- the two
// stages ran one after the other in every launch with a K-strided operand (dgrad, wgrad), one memory round trip per K step.  Inlining
// through a __restrict__ parameter attaches a scope to the builtin's call, and the wait goes away (tools/isa_loadchain.py: the loop
// reads `D D D D w0 |` instead of `D D D D w0 ... w0 |`).  The wait was never needed: a stage is read only after the barrier that
// follows the vmcnt(0) of the step that filled it.
template <int KMAJOR>
MH_DEV h16x8 read_frag_scoped(const char* __restrict__ lds, int rb, int kk, int lane) {
    return read_frag<KMAJOR>(lds, rb, kk, lane);
}

// f32 staging tile [rows][128]: the accumulator layout makes the four 16-lane groups of a wave write rows r, r+4, r+8,
// r+12 of the SAME 16 columns -- with 512-B rows that is the same 16 banks four times.  The 16-column block index is
// therefore XOR-ed with (row >> 2) & 3: the four groups land on four different 16-bank quarters (conflict-free), and a
// row-wise 32-B read stays inside one (permuted) block.  Odd rows also swap the two 16-B halves of every 32 B, so the
// 16-B epilogue reads of rows r and r+1 (one ds_read_b128 lane group spans both) use different banks.
MH_DEV int cs_index(int row, int col) { return row * BN + (col ^ (((row >> 2) & 3) << 4) ^ ((row & 1) << 2)); }

// ---- tile order: local tile index -> (row tile, column tile) -----------------------------------
// n-fastest order makes the ~64 tiles an XCD runs at once span 3-4 row panels x ALL column tiles: every K step touches the whole
// of B (3.5-4.7 MB at N = 2304 / 3072, K = 768), which together with the A panels overflows the XCD's 4-MB L2.  Blocked order:
// GROUP_M row panels x 8 column tiles at once = 8 + 8 operand panels, each re-used 8 times while it is hot.
MH_DEV void tile_coords(int tiles_n, int tiles_m, int group_m, int lt, int& tm, int& tn) {
    if (group_m <= 1) {
        tm = lt / tiles_n;
        tn = lt % tiles_n;
        return;
    }
    const int per_group = group_m * tiles_n;
    const int g = lt / per_group;
    const int r = lt - g * per_group;
    const int rows = min(group_m, tiles_m - g * group_m);
    tn = r / rows;
    tm = g * group_m + (r - tn * rows);
}

// GROUP_M of the tile order (0 / 1: n-fastest) for both kernels: 8 (measured in the step with the live-tile order: 8 -> 9.70-9.73 ms,
// 4 -> 9.90-9.91, 16 -> 9.78, 6 -> 9.92; tools/lab/RESULTS.md)
constexpr int GROUP_M = 8;

// ---- split-K: K cut into `splits` chunks of whole K tiles -----------------------------------
inline int ksplit_chunk(int K, int splits) { return ((K + splits - 1) / splits + BK - 1) / BK * BK; }
// the largest split count <= want whose every chunk holds part of K (the chunks are whole K tiles, so a count can leave the last empty)
inline int ksplit_fit(int K, int want) {
    for (int sp = want; sp > 1; --sp) {
        const int kc = ksplit_chunk(K, sp);
        if ((K + kc - 1) / kc == sp) return sp;
    }
    return 1;
}

// ---- the K loop ---------------------------------------------------------------------------------
struct NoHook {
    template <class... T>
    MH_DEV void operator()(T&&...) const {}
};

// acc = this wave's NI x NJ accumulators over nk K tiles.  issue(kt, stage) starts the LDS-DMA of K tile kt into `stage` (A image at
// stage, B image at stage + BM * BK * 2); two stages alternate, the next one issued before the MFMAs of the current one, ONE barrier
// per K tile.  a_hook(fa) runs after each 32-deep k-step's MFMAs with its A fragments; landed() right after the first stage's barrier.
// SCOPED: fragment reads through read_frag_scoped (gemm_kernel; conv_gemm_kernel keeps the plain ones until it has its own A/B).
template <int LA, int LB, bool SCOPED = false, class Issue, class AHook = NoHook, class Landed = NoHook>
MH_DEV void k_loop(f32x4 (&acc)[NI][NJ], char* smem, int nk, int wave, int lane, Issue issue, AHook a_hook = {}, Landed landed = {}) {
    const int wm0 = wave_m0(wave), wn0 = wave_n0(wave);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nk > 0) issue(0, smem);
    __syncthreads();
    landed();
    for (int kt = 0; kt < nk; ++kt) {
        char* cur = smem + (kt & 1) * STAGE_BYTES;
        char* nxt = smem + ((kt + 1) & 1) * STAGE_BYTES;
        if (kt + 1 < nk) issue(kt + 1, nxt);
        const char* la = cur;
        const char* lb = cur + BM * BK * 2;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            h16x8 fa[NI], fb[NJ];
#pragma unroll
            for (int i = 0; i < NI; ++i) fa[i] = SCOPED ? read_frag_scoped<LA>(la, wm0 + i * 16, kk, lane) : read_frag<LA>(la, wm0 + i * 16, kk, lane);
#pragma unroll
            for (int j = 0; j < NJ; ++j) fb[j] = SCOPED ? read_frag_scoped<LB>(lb, wn0 + j * 16, kk, lane) : read_frag<LB>(lb, wn0 + j * 16, kk, lane);
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = MH_MFMA_16x16x32(fa[i], fb[j], acc[i][j], 0, 0, 0);
            a_hook(fa);
        }
        __syncthreads();
    }
}

// accumulators -> f32 staging tile cs (the K loop ended with a barrier; the caller syncs before reading cs)
MH_DEV void stage_acc(float* cs, const f32x4 (&acc)[NI][NJ], int wave, int lane) {
    const int wm0 = wave_m0(wave), wn0 = wave_n0(wave);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                cs[cs_index(wm0 + i * 16 + (lane >> 4) * 4 + r, wn0 + j * 16 + (lane & 15))] = acc[i][j][r];
}

// split-K partial: alpha * the staged tile -> rows m0.., columns n0.. of one f32 slab [M][ldc] (rows past M / columns past N skipped)
MH_DEV void store_slab(float* slab, const float* cs, float alpha, int m0, int n0, int M, int N, int ldc, int tid) {
#pragma unroll
    for (int it = 0; it < BM * 16 / (NW * 64); ++it) {
        const int q = it * NW * 64 + tid;
        const int row = q >> 4, cc = q & 15;
        const int gm = m0 + row, gn = n0 + cc * 8;
        if (gm >= M || gn >= N) continue;
        const f32x4 x0 = *(const f32x4*)(cs + cs_index(row, cc * 8));
        const f32x4 x1 = *(const f32x4*)(cs + cs_index(row, cc * 8 + 4));
        float* c = slab + (size_t)gm * ldc + gn;
        *(f32x4*)c = x0 * alpha;
        *(f32x4*)(c + 4) = x1 * alpha;
    }
}

}  // namespace mh_tile
