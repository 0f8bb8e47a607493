// Depthwise k x k convolution (stride 1, padding k/2, bias) on NHWC 16-bit activations for gfx950: the spatial-mixing layer of a
// ConvNeXt block (torchvision CNBlock: Conv2d(dim, dim, 7, padding=3, groups=dim)), used by the forward-only feature extractor of
// the SVM baseline (baselines/extract_feat.py:52-60, 82-85).  See include/memehip.h (mh_dwconv_nhwc).  Further down, its backward for the
// trainable tower (convnext.ConvNeXtTiny.tower): the input gradient (the forward body, dwconv_tile.inc, with reversed taps), the weight /
// bias gradient (slab partials + a fixed-order finish) and the layer-scale gradient of the block's folded second Linear.
//
// HBM-bound (49 MACs per element against 4 bytes of traffic: 12 flop/B, far under the VALU ridge), so the design is about reading
// every activation once: a workgroup owns a T x T tile of output pixels x a chunk of <= 192 channels of one image and stages the
// (T+k-1)^2 halo tile in LDS (16-byte chunks, zero outside the image); a thread owns one OUTPUT ROW of the tile x 8 channels:
// per filter row it pulls the T+k-1 input pixels of that row into registers once and slides the k taps over them (each weight
// vector -- 8 channels, f32, from the [k*k][C] tap-major weight image, L1-resident -- is loaded once per tap and used T times).
// Consecutive threads take consecutive 8-channel groups: LDS reads and global stores are contiguous 16-byte runs.
#include "common.h"

namespace {

template <int T, int KS>
__global__ __launch_bounds__(256) void dwconv_kernel(const h16* __restrict__ x, const float* __restrict__ wt,
                                                     const float* __restrict__ bias, h16* __restrict__ y, int H, int W, int C,
                                                     int CB, int tiles_x) {
#define DW_DGRAD 0
#include "dwconv_tile.inc"
#undef DW_DGRAD
}

// the input gradient (see dwconv_tile.inc): x is dy, y is dx
template <int T, int KS>
__global__ __launch_bounds__(256) void dwconv_dgrad_kernel(const h16* __restrict__ x, const float* __restrict__ wt,
                                                           const h16* __restrict__ addend, h16* __restrict__ y, int H, int W, int C,
                                                           int CB, int tiles_x) {
#define DW_DGRAD 1
#include "dwconv_tile.inc"
#undef DW_DGRAD
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------
// dw[c][ky][kx] = sum_{b,h,w} dy[b][h][w][c] * x[b][h+ky-k/2][w+kx-k/2][c], dbias[c] = sum dy.  HBM-bound like the forward, so x and dy
// are read once: a workgroup owns a channel chunk (<= 96) and walks a SLAB of consecutive (image, tile) units; per unit it stages
// the x halo tile and the dy tile in LDS as the forward does.  A thread owns one FILTER ROW ky x 8 channels (k taps x 8 = 56 f32
// accumulators, kept in registers over the whole slab) and every RH-th output row of the tile: per output row it pulls the T dy
// pixels and the T+k-1 x pixels of halo row r+ky into registers once and slides the k taps over them.  After the slab the RH row
// shares are added through LDS in the order 0, 1, .. RH-1 and the workgroup writes ONE partial [k*k + 1][CB] (last row: dbias)
// into the workspace; dwconv_wgrad_finish_kernel sums the slabs in a fixed order.  No atomics: bit-identical from run to run.
template <int T, int KS>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const h16* __restrict__ x, const h16* __restrict__ dy, float* __restrict__ ws,
                                                           int H, int W, int C, int CB, int RH, int tiles_x, int tiles, int per,
                                                           int units) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HT = T + KS - 1, PAD = KS / 2, KK = KS * KS;
    const int groups = CB / 8;
    const int tid = threadIdx.x, nthr = groups * KS * RH;      // blockDim.x == nthr
    const int c_chunk = blockIdx.y * CB;
    const int g = tid % groups, ky = (tid / groups) % KS, rh = tid / (groups * KS);
    char* sdy = smem + (size_t)HT * HT * CB * 2;
    float acc[KS][8], accb[8];
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) accb[e] = 0.f;
    const int u0 = blockIdx.x * per, u1 = min(u0 + per, units);
#pragma unroll 1
    for (int u = u0; u < u1; ++u) {
        const int b = u / tiles, t = u - b * tiles;
        const int ty0 = (t / tiles_x) * T, tx0 = (t % tiles_x) * T;
        const size_t img = (size_t)b * H * W * C + c_chunk;
        for (int q = tid; q < HT * HT * groups; q += nthr) {
            const int pix = q / groups, cg = q - pix * groups;
            const int iy = ty0 - PAD + pix / HT, ix = tx0 - PAD + pix % HT;
            i32x4 v = {0, 0, 0, 0};
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const i32x4*)(x + img + ((size_t)iy * W + ix) * C + cg * 8);
            *(i32x4*)(smem + ((size_t)pix * CB + cg * 8) * 2) = v;
        }
        for (int q = tid; q < T * T * groups; q += nthr) {
            const int pix = q / groups, cg = q - pix * groups;
            const int oy = ty0 + pix / T, ox = tx0 + pix % T;
            i32x4 v = {0, 0, 0, 0};
            if (oy < H && ox < W) v = *(const i32x4*)(dy + img + ((size_t)oy * W + ox) * C + cg * 8);
            *(i32x4*)(sdy + ((size_t)pix * CB + cg * 8) * 2) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = rh; r < T; r += RH) {
            Pack8 d[T], in[HT];
#pragma unroll
            for (int i = 0; i < T; ++i) d[i].v = *(const i32x4*)(sdy + ((size_t)(r * T + i) * CB + g * 8) * 2);
#pragma unroll
            for (int i = 0; i < HT; ++i) in[i].v = *(const i32x4*)(smem + ((size_t)((r + ky) * HT + i) * CB + g * 8) * 2);
#pragma unroll
            for (int i = 0; i < T; ++i) {
                float dv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) dv[e] = mh_bf2f(d[i].e[e]);
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[kx][e] = fmaf(dv[e], mh_bf2f(in[i + kx].e[e]), acc[kx][e]);
                if (ky == 0) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) accb[e] += dv[e];
                }
            }
        }
        __syncthreads();
    }
    // the RH row shares of one (ky, channel group), added in the order 0 + 1 + ... through LDS (the staging space is free now)
    float* red = (float*)smem;      // [KK + 1][CB]
    for (int p = 1; p < RH; ++p) {
        if (rh == p) {
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                float* o = red + (size_t)(ky * KS + kx) * CB + g * 8;
                *(f32x4*)o = f32x4{acc[kx][0], acc[kx][1], acc[kx][2], acc[kx][3]};
                *(f32x4*)(o + 4) = f32x4{acc[kx][4], acc[kx][5], acc[kx][6], acc[kx][7]};
            }
            if (ky == 0) {
                float* o = red + (size_t)KK * CB + g * 8;
                *(f32x4*)o = f32x4{accb[0], accb[1], accb[2], accb[3]};
                *(f32x4*)(o + 4) = f32x4{accb[4], accb[5], accb[6], accb[7]};
            }
        }
        __syncthreads();
        if (rh == 0) {
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                const float* o = red + (size_t)(ky * KS + kx) * CB + g * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[kx][e] += o[e];
            }
            if (ky == 0) {
                const float* o = red + (size_t)KK * CB + g * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) accb[e] += o[e];
            }
        }
        __syncthreads();
    }
    if (rh != 0) return;
    float* wb = ws + (size_t)blockIdx.x * (KK + 1) * C + c_chunk + g * 8;
#pragma unroll
    for (int kx = 0; kx < KS; ++kx) {
        float* o = wb + (size_t)(ky * KS + kx) * C;
        *(f32x4*)o = f32x4{acc[kx][0], acc[kx][1], acc[kx][2], acc[kx][3]};
        *(f32x4*)(o + 4) = f32x4{acc[kx][4], acc[kx][5], acc[kx][6], acc[kx][7]};
    }
    if (ky == 0) {
        float* o = wb + (size_t)KK * C;
        *(f32x4*)o = f32x4{accb[0], accb[1], accb[2], accb[3]};
        *(f32x4*)(o + 4) = f32x4{accb[4], accb[5], accb[6], accb[7]};
    }
}

// the slab partials ws[n_slabs][KK + 1][C] -> dw (torch layout [C][1][k][k]) and dbias [C], times `scale`: a lane owns one (tap, channel),
// the four waves take every fourth slab and are added in wave order through LDS -- a fixed order
__global__ __launch_bounds__(256) void dwconv_wgrad_finish_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                  float* __restrict__ dbias, int n_slabs, int C, int KK, float scale,
                                                                  int accum) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = (KK + 1) * C, idx = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (idx < n)
        for (int sl = wave; sl < n_slabs; sl += 4) s += ws[(size_t)sl * n + idx];
    red[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || idx >= n) return;
    const float t = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) * scale;
    const int tap = idx / C, c = idx - tap * C;
    float* o = tap < KK ? dw + (size_t)c * KK + tap : (dbias ? dbias + c : nullptr);
    if (o) *o = accum ? *o + t : t;
}

// layer_scale backward over the FOLDED second Linear (W' = gamma W, b' = gamma b; dWp = dout^T h, dbp = colsum(dout)):
// dgamma[c] = sum_k W[c][k] dWp[c][k] + b[c] dbp[c], dW = gamma[c] dWp, db = gamma[c] dbp.  One wave per row c.
__global__ __launch_bounds__(256) void layer_scale_bwd_kernel(const float* __restrict__ Wm, const float* __restrict__ b,
                                                              const float* __restrict__ gamma, const float* dWp, const float* dbp,
                                                              float* dW, float* db, float* __restrict__ dgamma, int C, int K,
                                                              int accum) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= C) return;      // (wave-uniform)
    const float gm = gamma[row];
    const size_t base = (size_t)row * K;
    float s = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 w = *(const f32x4*)(Wm + base + k), d = *(const f32x4*)(dWp + base + k);
        s += (w[0] * d[0] + w[1] * d[1]) + (w[2] * d[2] + w[3] * d[3]);
        f32x4 o = d * gm;
        if (accum) o += *(const f32x4*)(dW + base + k);
        *(f32x4*)(dW + base + k) = o;
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float dbv = dbp[row];
        s += b[row] * dbv;
        dgamma[row] = accum ? dgamma[row] + s : s;
        db[row] = accum ? db[row] + gm * dbv : gm * dbv;
    }
}

// torch depthwise weight f32 [C][1][k][k] -> tap-major f32 [k*k][C] (what the kernel reads: 8 channels of one tap = 32 contiguous bytes)
__global__ __launch_bounds__(256) void dwconv_weight_pack_kernel(const float* __restrict__ w, float* __restrict__ wt, int C, int KK) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * KK) return;
    const int tap = idx / C, c = idx - tap * C;
    wt[idx] = w[(size_t)c * KK + tap];
}

template <int T, int KS>
int launch_dw(const h16* x, const float* wt, const float* bias, h16* y, int B, int H, int W, int C, hipStream_t s) {
    // channel chunk: the largest divisor of C that is a multiple of 8, <= 192 (LDS: (T+k-1)^2 x 192 x 2 B <= 75 KB) and keeps
    // the workgroup at <= 256 threads
    int CB = 0;
    for (int cb = 8; cb <= C && cb <= 192; cb += 8)
        if (C % cb == 0 && (cb / 8) * T <= 256) CB = cb;
    if (!CB) return MH_ESHAPE;
    constexpr int HT = T + KS - 1;
    const int lds = HT * HT * CB * 2;
    static int lds_set = 0;
    if (lds > lds_set) {
        (void)hipFuncSetAttribute((const void*)dwconv_kernel<T, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
        lds_set = 160 * 1024;
    }
    const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
    hipLaunchKernelGGL((dwconv_kernel<T, KS>), dim3(tiles_x * tiles_y, C / CB, B), dim3((CB / 8) * T), lds, s, x, wt, bias, y, H, W, C,
                       CB, tiles_x);
    return mh_launch_status();
}

template <int T, int KS>
int launch_dw_dgrad(const h16* dy, const float* wt, const h16* addend, h16* dx, int B, int H, int W, int C, hipStream_t s) {
    int CB = 0;      // the forward's chunk rule
    for (int cb = 8; cb <= C && cb <= 192; cb += 8)
        if (C % cb == 0 && (cb / 8) * T <= 256) CB = cb;
    if (!CB) return MH_ESHAPE;
    constexpr int HT = T + KS - 1;
    const int lds = HT * HT * CB * 2;
    static int lds_set = 0;
    if (lds > lds_set) {
        (void)hipFuncSetAttribute((const void*)dwconv_dgrad_kernel<T, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
        lds_set = 160 * 1024;
    }
    const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
    hipLaunchKernelGGL((dwconv_dgrad_kernel<T, KS>), dim3(tiles_x * tiles_y, C / CB, B), dim3((CB / 8) * T), lds, s, dy, wt, addend, dx, H,
                       W, C, CB, tiles_x);
    return mh_launch_status();
}

// 7-pixel tiles where they divide the image and 8-pixel ones do not (28, 14, 7), 8-pixel tiles otherwise (56)
bool dw_tile7(int H, int W) { return (H % 8) && (W % 8) && !(H % 7) && !(W % 7); }

// The weight gradient's launch plan, shared by the launcher and the workspace query.  Channel chunk: the largest divisor of C that is a
// multiple of 8 and <= 96 (LDS: x halo + dy tile, (14^2 + 8^2) x 96 x 2 B = 49 KB -- three workgroups per CU); RH row shares fill the
// workgroup up to 256 threads; the B x tiles units are cut into slabs so that about WGRAD_WORKGROUPS workgroups run.
constexpr int WGRAD_WORKGROUPS = 512;
struct WgradPlan {
    int T, CB, RH, tiles_x, tiles, per, n_slabs, units;
};
bool wgrad_plan(int B, int H, int W, int C, int K, WgradPlan& p) {
    if (B < 1 || H < 1 || W < 1 || C < 8 || (C % 8) || B > 65535 || K != 7) return false;
    if ((int64_t)B * H * W > (int64_t)1 << 30) return false;
    p.T = dw_tile7(H, W) ? 7 : 8;
    p.CB = 0;
    for (int cb = 8; cb <= C && cb <= 96; cb += 8)
        if (C % cb == 0) p.CB = cb;
    const int rows = (p.CB / 8) * K;      // <= 84 threads per row share
    p.RH = 256 / rows < p.T ? 256 / rows : p.T;
    p.tiles_x = (W + p.T - 1) / p.T;
    p.tiles = p.tiles_x * ((H + p.T - 1) / p.T);
    p.units = B * p.tiles;
    const int chunks = C / p.CB;
    const int want = WGRAD_WORKGROUPS / chunks > 1 ? WGRAD_WORKGROUPS / chunks : 1;
    p.per = (p.units + want - 1) / want;
    p.n_slabs = (p.units + p.per - 1) / p.per;
    return true;
}

template <int T, int KS>
int launch_dw_wgrad(const h16* x, const h16* dy, float* ws, const WgradPlan& p, int H, int W, int C, hipStream_t s) {
    constexpr int HT = T + KS - 1;
    const int lds = (HT * HT + T * T) * p.CB * 2;      // (>= the (KS*KS + 1) x CB f32 of the row-share reduction)
    hipLaunchKernelGGL((dwconv_wgrad_kernel<T, KS>), dim3(p.n_slabs, C / p.CB), dim3((p.CB / 8) * KS * p.RH), lds, s, x, dy, ws, H, W, C,
                       p.CB, p.RH, p.tiles_x, p.tiles, p.per, p.units);
    return mh_launch_status();
}

}  // namespace

extern "C" int mh_dwconv_weight_pack(const float* w, float* wt, int C, int K, mh_stream_t stream) {
    if (!w || !wt) return MH_EINVAL;
    if (C < 1 || K < 1) return MH_ESHAPE;
    hipLaunchKernelGGL(dwconv_weight_pack_kernel, dim3((C * K * K + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, wt, C, K * K);
    return mh_launch_status();
}

extern "C" int mh_dwconv_nhwc(const void* x, const float* wt, const float* bias, void* y, int B, int H, int W, int C, int K,
                              mh_stream_t stream) {
    if (!x || !wt || !y) return MH_EINVAL;
    if (B < 1 || H < 1 || W < 1 || C < 8 || (C % 8) || B > 65535) return MH_ESHAPE;
    if (K != 7) return MH_ESHAPE;      // ConvNeXt's 7 x 7 is the one filter size the path has
    hipStream_t s = (hipStream_t)stream;
    if (dw_tile7(H, W)) return launch_dw<7, 7>((const h16*)x, wt, bias, (h16*)y, B, H, W, C, s);
    return launch_dw<8, 7>((const h16*)x, wt, bias, (h16*)y, B, H, W, C, s);
}

extern "C" int mh_dwconv_nhwc_dgrad(const void* dy, const float* wt, const void* addend, void* dx, int B, int H, int W, int C, int K,
                                    mh_stream_t stream) {
    if (!dy || !wt || !dx) return MH_EINVAL;
    if (B < 1 || H < 1 || W < 1 || C < 8 || (C % 8) || B > 65535) return MH_ESHAPE;
    if (K != 7) return MH_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (dw_tile7(H, W)) return launch_dw_dgrad<7, 7>((const h16*)dy, wt, (const h16*)addend, (h16*)dx, B, H, W, C, s);
    return launch_dw_dgrad<8, 7>((const h16*)dy, wt, (const h16*)addend, (h16*)dx, B, H, W, C, s);
}

extern "C" int64_t mh_dwconv_wgrad_workspace_elems(int B, int H, int W, int C, int K) {
    WgradPlan p;
    if (!wgrad_plan(B, H, W, C, K, p)) return 0;
    return (int64_t)p.n_slabs * (K * K + 1) * C;
}

extern "C" int mh_dwconv_nhwc_wgrad(const void* x, const void* dy, float* dw, float* dbias, float* workspace, int B, int H, int W, int C,
                                    int K, float scale, int accum, mh_stream_t stream) {
    if (!x || !dy || !dw || !workspace) return MH_EINVAL;
    WgradPlan p;
    if (!wgrad_plan(B, H, W, C, K, p)) return MH_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int st = p.T == 7 ? launch_dw_wgrad<7, 7>((const h16*)x, (const h16*)dy, workspace, p, H, W, C, s)
                            : launch_dw_wgrad<8, 7>((const h16*)x, (const h16*)dy, workspace, p, H, W, C, s);
    if (st != MH_OK) return st;
    const int n = (K * K + 1) * C;
    hipLaunchKernelGGL(dwconv_wgrad_finish_kernel, dim3((n + 63) / 64), dim3(256), 0, s, workspace, dw, dbias, p.n_slabs, C, K * K, scale,
                       accum);
    return mh_launch_status();
}

extern "C" int mh_layer_scale_bwd(const float* W, const float* b, const float* gamma, const float* dWp, const float* dbp, float* dW,
                                  float* db, float* dgamma, int C, int K, int accum, mh_stream_t stream) {
    if (!W || !b || !gamma || !dWp || !dbp || !dW || !db || !dgamma) return MH_EINVAL;
    if (C < 1 || K < 4 || (K % 4)) return MH_ESHAPE;
    if (accum && (dW == dWp || db == dbp)) return MH_EINVAL;      // in place overwrites; accumulating needs outputs of their own
    hipLaunchKernelGGL(layer_scale_bwd_kernel, dim3((C + 3) / 4), dim3(256), 0, (hipStream_t)stream, W, b, gamma, dWp, dbp, dW, db, dgamma,
                       C, K, accum);
    return mh_launch_status();
}
