// Grouped 3x3 convolution (ResNeXt-50 32x4d: conv2 of every bottleneck, 32 groups of 4 / 8 / 16 / 32 channels) for gfx950.
//
// The layer does 1 / groups of the dense multiply-adds on the same activation bytes, so it is bound by the traffic of x and y.  Through the
// dense 128x128 implicit-GEMM tile (block-diagonal weights) 128 / Cg of the MFMA work would be zeros; here one wave owns 16 output channels
// and contracts only over the channels of the groups those 16 columns belong to:
//   Cg <= 16: the 16 input channels [c0, c0 + 16) (the same 16-block: Cin == Cout and Cg | 16), TWO filter taps per K = 32 step of
//             mfma_f32_16x16x32 -- 5 steps for the 9 taps (the 10th half step is zero), the 16 x 16 weight of a tap block-diagonal;
//   Cg == 32: the 32 input channels of the one group, one tap per step -- 9 steps, no zero block.
// The products are taken TRANSPOSED (D[channel][pixel] = W . X^T: the weights are the A operand, the activations the B operand), so a lane
// ends up with 4 consecutive channels of one pixel -- one 8-byte store per lane -- and a channel's BatchNorm sums are a 16-lane butterfly.
// A wave keeps its 5 / 9 weight fragments in registers for a whole 128-row tile; every activation fragment is ONE 16-byte buffer load of
// (pixel + tap, 8 channels), padding and the empty tap read as zeros through the buffer bounds.  The four waves of a workgroup cover 64
// adjacent channels, i.e. whole 128-byte lines of x; a tile's 9-fold tap reuse is served by the L1 / L2, HBM sees x once.
// The input gradient is the same kernel: per INPUT pixel a gather over the taps that reach it (stride 2: those of matching parity), with the
// second image of the packed weight (each group's block transposed).
// The weight gradient contracts over pixels, so both operands go through LDS as [pixel][64 channels] and the fragments are read
// transposed, 16 bits at a time; units of 32 output pixels (RT rows x WT columns of one image) share one x halo.
#include "common.h"

namespace {

constexpr uint32_t OOB = 0x80000000u;      // (every tensor < 2 GiB: this offset is past any buffer's end, the load returns zeros)

struct GcArgs {
    int B, Hs, Ws;        // the tensor that is READ (forward: x; dgrad: dy)
    int Hd, Wd;           // the tensor that is WRITTEN
    int C, stride, Md, nblk;
    uint32_t src_bytes;
};

// f32 [C][Cg][3][3] -> two images of 16-bit MFMA A-fragments, [image][C / 16][NS][64 lanes][8]: lane l, element j of step s of 16-block
// cb is A[row = l & 15][k = 8 (l >> 4) + j].  k -> (tap, cc): Cg <= 16: tap = 2 s + (k >> 4), cc = k & 15, contraction channel
// 16 cb + cc; Cg == 32: tap = s, cc = k, contraction channel 32 (cb / 2) + cc.  Image 0 (forward): row = output channel, contraction =
// input channel.  Image 1 (dgrad): row = input channel, contraction = output channel.  Pairs of two groups and tap 9 are zeros.
__global__ __launch_bounds__(256) void gconv_pack_kernel(const float* __restrict__ w, h16* __restrict__ wk, int C, int Cg, int NS) {
    const int per = (C / 16) * NS * 512;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * per) return;
    const int img = idx / per;
    int t = idx - img * per;
    const int j = t & 7, lane = (t >> 3) & 63;
    t >>= 9;
    const int s = t % NS, cb = t / NS;
    const int k = 8 * (lane >> 4) + j, row = cb * 16 + (lane & 15);
    const int tap = NS == 5 ? 2 * s + (k >> 4) : s;
    const int con = NS == 5 ? cb * 16 + (k & 15) : (cb >> 1) * 32 + k;
    const int co = img ? con : row, ci = img ? row : con;
    float v = 0.f;
    if (tap < 9 && co / Cg == ci / Cg) v = w[((size_t)co * Cg + ci % Cg) * 9 + tap];
    wk[idx] = (h16)v;
}

// One 128-row tile of the written tensor x 64 channels per workgroup; wave `wave` owns channels [16 cb, 16 cb + 16).
template <int NS, bool DGRAD>
__global__ __launch_bounds__(256) void gconv_kernel(const h16* __restrict__ src, const h16* __restrict__ wimg, h16* __restrict__ dst,
                                                    float* __restrict__ bn_part, GcArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cb = blockIdx.y * 4 + wave;
    if (cb * 16 >= a.C) return;      // (no barrier in this kernel)
    const int r = lane & 15, q = lane >> 4;
    Pack8 wf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) wf[s].v = *(const i32x4*)(wimg + ((size_t)(cb * NS + s) * 64 + lane) * 8);
    const int ch = NS == 5 ? cb * 16 + (q & 1) * 8 : (cb >> 1) * 32 + q * 8;
    const int tapsel = NS == 5 ? (q >> 1) : 0;
    const __amdgpu_buffer_rsrc_t rs = mh_rsrc(src, a.src_bytes);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int rg = 0; rg < 8; ++rg) {
        const int m = blockIdx.x * 128 + rg * 16 + r;
        const bool valid = m < a.Md;
        const int wd = m % a.Wd, t = m / a.Wd;
        const int hd = t % a.Hd, b = t / a.Hd;
        Pack8 xf[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int tap = NS == 5 ? 2 * s + tapsel : s;
            const int kh = tap / 3, kw = tap - 3 * kh;
            int hs, ws;
            bool ok = valid && tap < 9;
            if (DGRAD) {      // the outputs (hs, ws) with hs * stride - 1 + kh == hd
                const int th = hd + 1 - kh, tw = wd + 1 - kw;
                ok = ok && th >= 0 && tw >= 0;
                if (a.stride == 2) {
                    ok = ok && !((th | tw) & 1);
                    hs = th >> 1, ws = tw >> 1;
                } else {
                    hs = th, ws = tw;
                }
                ok = ok && hs < a.Hs && ws < a.Ws;
            } else {
                hs = hd * a.stride - 1 + kh, ws = wd * a.stride - 1 + kw;
                ok = ok && hs >= 0 && ws >= 0 && hs < a.Hs && ws < a.Ws;
            }
            const uint32_t off = ok ? (uint32_t)((((b * a.Hs + hs) * a.Ws + ws) * a.C + ch) * 2) : OOB;
            xf[s].v = mh_buf_load16(rs, off);
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = MH_MFMA_16x16x32(wf[s].h, xf[s].h, acc, 0, 0, 0);
        // acc[i]: channel 16 cb + 4 q + i of pixel m
        Pack4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o.e[i] = (h16)acc[i];
            const float v = (float)o.e[i];      // the value as stored (rows past Md are exact zeros)
            s1[i] += v;
            s2[i] += v * v;
        }
        if (valid) *(i32x2*)(dst + (size_t)m * a.C + cb * 16 + 4 * q) = o.v;
    }
    if (!DGRAD && bn_part) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float u = s1[i], v = s2[i];
            u += mh_xor_partner<8>(u, lane), v += mh_xor_partner<8>(v, lane);
            u += mh_xor_partner<4>(u, lane), v += mh_xor_partner<4>(v, lane);
            u += mh_xor_partner<2>(u, lane), v += mh_xor_partner<2>(v, lane);
            u += mh_xor_partner<1>(u, lane), v += mh_xor_partner<1>(v, lane);
            if (r == 0) {
                const int c = cb * 16 + 4 * q + i;
                bn_part[(size_t)c * a.nblk + blockIdx.x] = u;
                bn_part[(size_t)(a.C + c) * a.nblk + blockIdx.x] = v;
            }
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------
constexpr int WG_WORKGROUPS = 512;
constexpr int WG_PITCH = 66;             // 16-bit elements per staged pixel: 64 channels + one dword (33 dwords: 8 pixels apart = 8 banks apart)
constexpr int WG_XPIX = 195;             // the largest x halo of a unit: 3 x 65 pixels (1 x 32 outputs, stride 2)
struct WgPlan {
    int Ho, Wo, WT, RT, wshift, segs, rblks, units, per, chunks, XR, XC;
};
bool wg_plan(int B, int H, int W, int C, int stride, WgPlan& p) {
    p.Ho = (H - 1) / stride + 1, p.Wo = (W - 1) / stride + 1;      // (H + 2 - 3) / stride + 1
    // a unit = 32 output pixels as RT rows x WT columns, 1 x 32, 2 x 16 or 4 x 8: the shape with the least to stage over the image, empty
    // slots included (56 x 56 / stride 1: 98 units of 4 x 8 with a 6 x 10 halo, against 112 of 1 x 32 with a 3 x 34 halo)
    int64_t best = -1;
    for (int ws = 3; ws <= 5; ++ws) {
        const int WT = 1 << ws, RT = 32 >> ws;
        const int64_t n = (int64_t)((p.Wo + WT - 1) / WT) * ((p.Ho + RT - 1) / RT);
        const int64_t cost = n * (((RT - 1) * stride + 3) * ((WT - 1) * stride + 3) + 32);
        if (best < 0 || cost < best) best = cost, p.wshift = ws;
    }
    p.WT = 1 << p.wshift, p.RT = 32 >> p.wshift;
    p.segs = (p.Wo + p.WT - 1) / p.WT, p.rblks = (p.Ho + p.RT - 1) / p.RT;
    const int64_t units = (int64_t)B * p.rblks * p.segs;
    if (units > (1 << 24)) return false;
    p.units = (int)units;
    const int bundles = (C + 63) / 64;
    const int want = WG_WORKGROUPS / bundles > 1 ? WG_WORKGROUPS / bundles : 1;
    p.per = (p.units + want - 1) / want;
    p.chunks = (p.units + p.per - 1) / p.per;
    p.XR = (p.RT - 1) * stride + 3, p.XC = (p.WT - 1) * stride + 3;
    return p.XR * p.XC <= WG_XPIX;
}

struct WgArgs {
    int B, H, W, C, Cg, stride;
    uint32_t x_bytes, dy_bytes;
    WgPlan p;
};

// grid (chunks, ceil(C / 64)).  part[chunk][C][Cg][9] f32: every element written by exactly one lane.
// S: the stride.  A lane's 8 pixel slots lie in one row of the unit (WT >= 8), so for one filter row its 24 operands (8 slots x 3 taps)
// are only 7 S + 3 distinct pixels of the halo: each is read from LDS once and the three taps' fragments are put together in registers.
// Cg <= 16: the next unit's global loads are issued before this unit's MFMAs (registers: 1 + NL x 16 bytes), so their latency is not on
// the barrier-to-barrier path; Cg == 32 holds 72 accumulator registers and loads at the top of the unit instead.
template <bool CG32, int S>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(const h16* __restrict__ dy, const h16* __restrict__ x, float* __restrict__ part,
                                                          WgArgs a) {
    __shared__ uint32_t xs[WG_XPIX * 33];
    __shared__ uint32_t dys[32 * 33];
    const h16* xs16 = (const h16*)xs;
    const h16* dys16 = (const h16*)dys;
    const WgPlan& p = a.p;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, q = lane >> 4;
    const int cbase = blockIdx.y * 64, cb = blockIdx.y * 4 + wave;
    const bool active = cb * 16 < a.C;
    const int cib = CG32 ? (wave >> 1) * 32 : wave * 16;      // first x channel (within the 64) of this wave's contraction
    const __amdgpu_buffer_rsrc_t rx = mh_rsrc(x, a.x_bytes), rdy = mh_rsrc(dy, a.dy_bytes);
    // the halo pixel of this lane's first slot (k = 8 q) at tap (0, 0); slot 8 q + j is S j pixels to its right
    const int pix0 = (((8 * q) >> p.wshift) * S) * p.XC + ((8 * q) & (p.WT - 1)) * S;
    constexpr int NB = CG32 ? 2 : 1;
    constexpr int NL = S == 1 ? 4 : 7;      // x chunks per thread: ceil(102 * 8 / 256), ceil(195 * 8 / 256) (the largest halo per stride)
    constexpr int NV = 7 * S + 3;
    f32x4 acc[9][NB];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int h = 0; h < NB; ++h) acc[t][h] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int u0 = blockIdx.x * p.per, u1 = u0 + p.per < p.units ? u0 + p.per : p.units;
    const int c8 = (tid & 7) * 8;
    const bool chan_ok = cbase + c8 < a.C;
    const int npix = p.XR * p.XC;
    i32x4 pdy, px[NL];
    auto issue = [&](int u) {      // the global loads of unit u: one dy chunk (32 slots x 8 chunks of 8 channels) and <= NL halo chunks per thread
        const int seg = u % p.segs, t = u / p.segs;
        const int rb = t % p.rblks, b = t / p.rblks;
        const int ho0 = rb * p.RT, wo0 = seg * p.WT;
        const int hi0 = ho0 * S - 1, wi0 = wo0 * S - 1;
        const int slot = tid >> 3;
        const int ho = ho0 + (slot >> p.wshift), wo = wo0 + (slot & (p.WT - 1));
        const bool okd = chan_ok && ho < p.Ho && wo < p.Wo;
        pdy = mh_buf_load16(rdy, okd ? (uint32_t)((((b * p.Ho + ho) * p.Wo + wo) * a.C + cbase + c8) * 2) : OOB);
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int pix = (tid >> 3) + 32 * k;      // (past npix: loaded as zeros, not written)
            const int xr = pix / p.XC, xc = pix - xr * p.XC;
            const int hi = hi0 + xr, wi = wi0 + xc;
            const bool ok = chan_ok && pix < npix && hi >= 0 && wi >= 0 && hi < a.H && wi < a.W;
            px[k] = mh_buf_load16(rx, ok ? (uint32_t)((((b * a.H + hi) * a.W + wi) * a.C + cbase + c8) * 2) : OOB);
        }
    };
    if (!CG32 && u0 < u1) issue(u0);
    for (int u = u0; u < u1; ++u) {
        if (CG32) issue(u);
        {
            uint32_t* d = dys + (tid >> 3) * 33 + (c8 >> 1);
            d[0] = pdy[0], d[1] = pdy[1], d[2] = pdy[2], d[3] = pdy[3];
        }
#pragma unroll
        for (int k = 0; k < NL; ++k) {      // the x halo, every pixel of it (zeros outside the image)
            const int pix = (tid >> 3) + 32 * k;
            if (pix < npix) {
                uint32_t* d = xs + pix * 33 + (c8 >> 1);
                d[0] = px[k][0], d[1] = px[k][1], d[2] = px[k][2], d[3] = px[k][3];
            }
        }
        __syncthreads();
        if (!CG32 && u + 1 < u1) issue(u + 1);
        if (active) {
            Pack8 fa;      // A[row = output channel r][k = pixel slot]
#pragma unroll
            for (int j = 0; j < 8; ++j) fa.e[j] = dys16[(8 * q + j) * WG_PITCH + wave * 16 + r];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
                for (int h = 0; h < NB; ++h) {
                    h16 v[NV];
#pragma unroll
                    for (int o = 0; o < NV; ++o) v[o] = xs16[(pix0 + kh * p.XC + o) * WG_PITCH + cib + 16 * h + r];
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        Pack8 fb;      // B[k = pixel slot][column = input channel r]
#pragma unroll
                        for (int j = 0; j < 8; ++j) fb.e[j] = v[j * S + kw];
                        acc[3 * kh + kw][h] = MH_MFMA_16x16x32(fa.h, fb.h, acc[3 * kh + kw][h], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    // acc[tap][h][i]: output channel 16 cb + 4 q + i, input channel (of the 16-block, or of half h of the group) r
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = cb * 16 + 4 * q + i;
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            const int cil = CG32 ? 16 * h + r : r % a.Cg;
            const bool same = CG32 || (r / a.Cg == (4 * q + i) / a.Cg);
            if (!same) continue;
            float* d = part + (((size_t)blockIdx.x * a.C + co) * a.Cg + cil) * 9;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) d[tap] = acc[tap][h][i];
        }
    }
}

__global__ __launch_bounds__(256) void gconv_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ dw, int n, int chunks,
                                                                 float alpha, int accumulate) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * n + idx];      // chunk order: the same bits on every run
    const float v = __fmul_rn(alpha, s);
    dw[idx] = accumulate ? __fadd_rn(dw[idx], v) : v;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the one geometry rule of every entry point
int gc_check(const MhConvGeom* g, int groups) {
    if (g->B < 1 || g->H < 1 || g->W < 1 || g->C < 32 || (g->C % 32) || g->Cout != g->C) return MH_ESHAPE;
    if (groups < 1 || g->C % groups) return MH_ESHAPE;
    const int cg = g->C / groups;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return MH_ESHAPE;
    if (g->KH != 3 || g->KW != 3 || g->pad != 1 || (g->stride != 1 && g->stride != 2)) return MH_ESHAPE;
    const int64_t M = (int64_t)g->B * g->H * g->W;
    if (M >= (1 << 24) || M * g->C * 2 >= ((int64_t)1 << 31)) return MH_ESHAPE;
    return MH_OK;
}

int gc_launch(const h16* src, const h16* wimg, h16* dst, float* bn_part, const MhConvGeom* g, int groups, bool dgrad, hipStream_t s) {
    const int Ho = (g->H - 1) / g->stride + 1, Wo = (g->W - 1) / g->stride + 1;
    GcArgs a;
    a.B = g->B, a.C = g->C, a.stride = g->stride;
    if (dgrad) a.Hs = Ho, a.Ws = Wo, a.Hd = g->H, a.Wd = g->W;
    else a.Hs = g->H, a.Ws = g->W, a.Hd = Ho, a.Wd = Wo;
    a.Md = a.B * a.Hd * a.Wd;
    a.nblk = (a.Md + 127) / 128;
    a.src_bytes = (uint32_t)((int64_t)a.B * a.Hs * a.Ws * a.C * 2);
    const dim3 grid(a.nblk, (g->C + 63) / 64);
    const bool cg32 = g->C / groups == 32;
    if (cg32 && dgrad) hipLaunchKernelGGL((gconv_kernel<9, true>), grid, dim3(256), 0, s, src, wimg, dst, bn_part, a);
    else if (cg32) hipLaunchKernelGGL((gconv_kernel<9, false>), grid, dim3(256), 0, s, src, wimg, dst, bn_part, a);
    else if (dgrad) hipLaunchKernelGGL((gconv_kernel<5, true>), grid, dim3(256), 0, s, src, wimg, dst, bn_part, a);
    else hipLaunchKernelGGL((gconv_kernel<5, false>), grid, dim3(256), 0, s, src, wimg, dst, bn_part, a);
    return mh_launch_status();
}

int64_t gc_image_elems(int C, int groups) { return (int64_t)(C / 16) * (C / groups == 32 ? 9 : 5) * 512; }

}  // namespace

extern "C" int mh_gconv_packed_elems(int C, int groups) {
    if (C < 32 || (C % 32) || groups < 1 || C % groups) return 0;
    const int cg = C / groups;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return 0;
    const int64_t n = 2 * gc_image_elems(C, groups);
    return n < ((int64_t)1 << 30) ? (int)n : 0;
}

extern "C" int mh_gconv_weight_pack(const float* w, void* wk, int C, int groups, mh_stream_t stream) {
    if (!w || !wk || !aligned(w, 4) || !aligned(wk, 16)) return MH_EINVAL;
    const int n = mh_gconv_packed_elems(C, groups);
    if (!n) return MH_ESHAPE;
    const int cg = C / groups;
    hipLaunchKernelGGL(gconv_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, (h16*)wk, C, cg,
                       cg == 32 ? 9 : 5);
    return mh_launch_status();
}

extern "C" int mh_gconv_fwd(const void* x, const void* wk, void* y, float* bn_part, const MhConvGeom* g, int groups, mh_stream_t stream) {
    if (!x || !wk || !y || !g || !aligned(x, 16) || !aligned(wk, 16) || !aligned(y, 16) || !aligned(bn_part, 4)) return MH_EINVAL;
    const int st = gc_check(g, groups);
    if (st != MH_OK) return st;
    return gc_launch((const h16*)x, (const h16*)wk, (h16*)y, bn_part, g, groups, false, (hipStream_t)stream);
}

extern "C" int mh_gconv_dgrad(const void* dy, const void* wk, void* dx, const MhConvGeom* g, int groups, mh_stream_t stream) {
    if (!dy || !wk || !dx || !g || !aligned(dy, 16) || !aligned(wk, 16) || !aligned(dx, 16)) return MH_EINVAL;
    const int st = gc_check(g, groups);
    if (st != MH_OK) return st;
    return gc_launch((const h16*)dy, (const h16*)wk + gc_image_elems(g->C, groups), (h16*)dx, nullptr, g, groups, true, (hipStream_t)stream);
}

extern "C" int mh_gconv_wgrad_workspace_elems(const MhConvGeom* g, int groups) {
    WgPlan p;
    if (!g || gc_check(g, groups) != MH_OK || !wg_plan(g->B, g->H, g->W, g->C, g->stride, p)) return 0;
    const int64_t n = (int64_t)p.chunks * g->C * (g->C / groups) * 9;
    return n < ((int64_t)1 << 31) ? (int)n : 0;
}

extern "C" int mh_gconv_wgrad(const void* dy, const void* x, float* dw, float* workspace, int accumulate, float alpha, const MhConvGeom* g,
                              int groups, mh_stream_t stream) {
    if (!dy || !x || !dw || !workspace || !g || !aligned(dy, 16) || !aligned(x, 16) || !aligned(dw, 4) || !aligned(workspace, 4))
        return MH_EINVAL;
    const int st = gc_check(g, groups);
    if (st != MH_OK) return st;
    WgArgs a;
    if (!wg_plan(g->B, g->H, g->W, g->C, g->stride, a.p)) return MH_ESHAPE;
    a.B = g->B, a.H = g->H, a.W = g->W, a.C = g->C, a.Cg = g->C / groups, a.stride = g->stride;
    a.x_bytes = (uint32_t)((int64_t)g->B * g->H * g->W * g->C * 2);
    a.dy_bytes = (uint32_t)((int64_t)g->B * a.p.Ho * a.p.Wo * g->C * 2);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a.p.chunks, (g->C + 63) / 64);
    const h16 *pdy = (const h16*)dy, *px = (const h16*)x;
    if (a.Cg == 32 && a.stride == 1) hipLaunchKernelGGL((gconv_wgrad_kernel<true, 1>), grid, dim3(256), 0, s, pdy, px, workspace, a);
    else if (a.Cg == 32) hipLaunchKernelGGL((gconv_wgrad_kernel<true, 2>), grid, dim3(256), 0, s, pdy, px, workspace, a);
    else if (a.stride == 1) hipLaunchKernelGGL((gconv_wgrad_kernel<false, 1>), grid, dim3(256), 0, s, pdy, px, workspace, a);
    else hipLaunchKernelGGL((gconv_wgrad_kernel<false, 2>), grid, dim3(256), 0, s, pdy, px, workspace, a);
    int rc = mh_launch_status();
    if (rc != MH_OK) return rc;
    const int n = g->C * a.Cg * 9;
    hipLaunchKernelGGL(gconv_wgrad_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, workspace, dw, n, a.p.chunks, alpha, accumulate);
    return mh_launch_status();
}
