// Squeeze-and-excitation (timm's SEModule behind a bottleneck's bn3; see include/memehip.h, "squeeze-and-excitation"):
//   u [B*HW][C] 16-bit -> pooled = mean_hw u (mh_avgpool_fwd, conv.hip) -> hidden = relu(fc1 pooled + b1) -> s = sigmoid(fc2 hidden + b2)
//   -> y = relu(u * s + shortcut), and the backward of that.  Everything indexed [B][C] / [B][R] is f32.
// Three streaming kernels over the activation (one 16-byte chunk of 8 channels per thread and trip, no LDS but for the column sums) and the
// gate's two tiny layers (<= 2 x 4096 x 256 weights): per (image, hidden unit) and per (image, channel) forward, per image / per hidden
// unit / per weight backward.  No atomics anywhere: every sum has ONE owner and an order that the shape alone fixes, so two calls give the same bits.
#include "common.h"

namespace {

constexpr int SE_MAX_C = 4096, SE_MAX_R = 256;
constexpr int SE_GATE_THREADS = 1024;      // the per-image backward gate kernel: 16 waves share one image's two layers

// eight consecutive f32 of a [B][C] row (32-byte aligned: C % 8 == 0) as two 16-byte loads
MH_DEV void se_load8(const float* __restrict__ p, float (&o)[8]) {
    const f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
}

// ---- streaming kernels: grid (256-thread blocks over one image's HW * C / 8 16-byte chunks, B): one chunk per thread ------------------
// y = relu(u * s[b] + shortcut): f32, one rounding
__global__ __launch_bounds__(256) void se_apply_fwd_kernel(const h16* __restrict__ u, const float* __restrict__ s, const h16* __restrict__ sc,
                                                           h16* __restrict__ y, uint32_t per, int C) {
    const uint32_t C8 = (uint32_t)C >> 3;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const size_t off = ((size_t)blockIdx.y * per + i) * 8;
    Pack8 a, r, o;
    a.v = *(const i32x4*)(u + off);
    r.v = *(const i32x4*)(sc + off);
    float sv[8];
    se_load8(s + (size_t)blockIdx.y * C + (i % C8) * 8, sv);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = mh_f2bf(fmaxf(fmaf(mh_bf2f(a.e[e]), sv[e], mh_bf2f(r.e[e])), 0.f));
    *(i32x4*)(y + off) = o.v;
}
// du = g * s[b] + dpooled[b] / HW: f32 (a true division: dpooled = k * HW gives exactly k), one rounding
__global__ __launch_bounds__(256) void se_apply_bwd_kernel(const h16* __restrict__ g, const float* __restrict__ s, const float* __restrict__ dp,
                                                           h16* __restrict__ du, uint32_t per, int C, float hw) {
    const uint32_t C8 = (uint32_t)C >> 3;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const size_t off = ((size_t)blockIdx.y * per + i) * 8, row = (size_t)blockIdx.y * C + (i % C8) * 8;
    Pack8 a, o;
    a.v = *(const i32x4*)(g + off);
    float sv[8], dv[8];
    se_load8(s + row, sv);
    se_load8(dp + row, dv);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = mh_f2bf(fmaf(mh_bf2f(a.e[e]), sv[e], dv[e] / hw));
    *(i32x4*)(du + off) = o.v;
}

// g = dy where y > 0 (dy's bits) else +0;  ds[b][c] = sum_hw g * u.  Grid (ceil(C / 64), B): ONE workgroup owns the 64 columns of an image
// over all of HW, so no partial leaves the launch.  Thread = (8-channel chunk tid & 7, row lane tid >> 3): a wave reads 8 rows x 128
// contiguous bytes.  Order of a column's sum: a thread's rows ascending (four rows' loads in flight per trip), then the wave's 8 row
// lanes by the xor butterfly 8 / 16 / 32, then the waves ascending.  Loads are branch-free (clamped address), masked where used.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void se_apply_bwd_reduce_kernel(const h16* __restrict__ dy, const h16* __restrict__ y,
                                                                      const h16* __restrict__ u, h16* __restrict__ g, float* __restrict__ ds,
                                                                      int HW, int C) {
    constexpr int RL = THREADS / 8, NW = THREADS / 64, UN = 4;
    __shared__ float red[NW][64];
    const int tid = threadIdx.x, c8 = blockIdx.x * 8 + (tid & 7), rl = tid >> 3;
    const bool on = c8 < (C >> 3);
    const size_t base = (size_t)blockIdx.y * HW * C + (size_t)min(c8, (C >> 3) - 1) * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int r0 = rl; r0 < HW; r0 += UN * RL) {
        Pack8 a[UN], m[UN], v[UN];
#pragma unroll
        for (int k = 0; k < UN; ++k) {
            const size_t off = base + (size_t)min(r0 + k * RL, HW - 1) * C;
            a[k].v = *(const i32x4*)(dy + off);
            m[k].v = *(const i32x4*)(y + off);
            v[k].v = *(const i32x4*)(u + off);
        }
#pragma unroll
        for (int k = 0; k < UN; ++k) {
            const bool ok = on && r0 + k * RL < HW;
            Pack8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool keep = ok && mh_bf2f(m[k].e[e]) > 0.f;
                o.e[e] = keep ? a[k].e[e] : (h16)0.f;
                acc[e] = fmaf(keep ? mh_bf2f(a[k].e[e]) : 0.f, mh_bf2f(v[k].e[e]), acc[e]);
            }
            if (ok) *(i32x4*)(g + base + (size_t)(r0 + k * RL) * C) = o.v;
        }
    }
    const unsigned lane = mh_lane_id();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] += mh_xor_partner<8>(acc[e], lane);
        acc[e] += mh_xor_partner<16>(acc[e], lane);
        acc[e] += mh_xor_partner<32>(acc[e], lane);
    }
    if (lane < 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[tid >> 6][lane * 8 + e] = acc[e];
    }
    __syncthreads();
    const int c = blockIdx.x * 64 + tid;
    if (tid < 64 && c < C) {
        float t = red[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += red[w][tid];
        ds[(size_t)blockIdx.y * C + c] = t;
    }
}

// ---- the gate -------------------------------------------------------------------------------------------------------------------
// the gradient at the pre-sigmoid activation: s (1 - s) is exactly 0 where s saturated to 1 and ~e^-|a| at the 0 side
MH_DEV float se_dgate(float ds, float s) { return ds * s * (1.0f - s); }

// hidden[b][r] = relu(w1[r] . pooled[b] + b1[r]): a wave per (b, r), lanes over c (coalesced rows of w1).  Grid (B, ceil(R / 4)).  (One
// workgroup per image walked both layers in 84 us at C = 2048, R = 128, batch 32 -- 32 workgroups, every dot product a dependent round trip.)
__global__ __launch_bounds__(256) void se_gate_hidden_kernel(const float* __restrict__ pooled, const float* __restrict__ w1,
                                                             const float* __restrict__ b1, float* __restrict__ hidden, int C, int R) {
    const int lane = threadIdx.x & 63, r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (r >= R) return;      // (the whole wave)
    const float* w = w1 + (size_t)r * C;
    const float* p = pooled + (size_t)blockIdx.x * C;
    float acc = 0.f;
#pragma unroll 8
    for (int c = lane; c < C; c += 64) acc = fmaf(w[c], p[c], acc);
    acc = wave_sum(acc);
    if (lane == 0) hidden[(size_t)blockIdx.x * R + r] = fmaxf(acc + b1[r], 0.f);
}
// s[b][c] = 1 / (1 + expf(-(w2[c] . hidden[b] + b2[c]))): a thread per (b, c) walks its own row of w2 (VEC: 16-byte loads, R % 4 == 0 and an
// aligned w2), hidden[b] in LDS.  Grid (B, ceil(C / 256)).  expf(+-large) is inf or 0, so a saturated gate is exactly 0 or 1: no NaN.
template <bool VEC>
__global__ __launch_bounds__(256) void se_gate_scale_kernel(const float* __restrict__ hidden, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, float* __restrict__ s, int C, int R) {
    __shared__ __attribute__((aligned(16))) float h[SE_MAX_R];
    const int tid = threadIdx.x, c = blockIdx.y * 256 + tid;
    const size_t b = blockIdx.x;
    if (tid < R) h[tid] = hidden[b * R + tid];
    __syncthreads();
    if (c >= C) return;
    const float* w = w2 + (size_t)c * R;
    float acc = 0.f;
    if (VEC) {
#pragma unroll 4
        for (int r = 0; r < R; r += 4) {
            const f32x4 v = *(const f32x4*)(w + r);
            acc = fmaf(v[0], h[r], acc);
            acc = fmaf(v[1], h[r + 1], acc);
            acc = fmaf(v[2], h[r + 2], acc);
            acc = fmaf(v[3], h[r + 3], acc);
        }
    } else {
#pragma unroll 4
        for (int r = 0; r < R; ++r) acc = fmaf(w[r], h[r], acc);
    }
    s[b * C + c] = 1.0f / (1.0f + expf(-(acc + b2[c])));
}

// dpooled, one workgroup per image: da = se_dgate into LDS; dh[r] = sum_c da[c] w2[c][r] by (group, r) threads (lanes over r: coalesced
// rows of w2; a group takes every G-th c, the groups are summed ascending), masked by hidden > 0; dpooled[c] = sum_r dh[r] w1[r][c].
__global__ __launch_bounds__(SE_GATE_THREADS) void se_gate_bwd_dpooled_kernel(const float* __restrict__ ds, const float* __restrict__ s,
                                                                              const float* __restrict__ hidden, const float* __restrict__ w1,
                                                                              const float* __restrict__ w2, float* __restrict__ dpooled,
                                                                              int C, int R) {
    __shared__ float da[SE_MAX_C];
    __shared__ float part[SE_GATE_THREADS];
    __shared__ float dh[SE_MAX_R];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    for (int c = tid; c < C; c += SE_GATE_THREADS) da[c] = se_dgate(ds[b * C + c], s[b * C + c]);
    __syncthreads();
    const int G = SE_GATE_THREADS / R, r = tid % R, grp = tid / R;
    if (grp < G) {
        float acc = 0.f;
#pragma unroll 4
        for (int c = grp; c < C; c += G) acc = fmaf(da[c], w2[(size_t)c * R + r], acc);
        part[grp * R + r] = acc;
    }
    __syncthreads();
    if (tid < R) {
        float t = part[tid];
        for (int k = 1; k < G; ++k) t += part[k * R + tid];
        dh[tid] = hidden[b * R + tid] > 0.f ? t : 0.f;
    }
    __syncthreads();
    for (int c = tid; c < C; c += SE_GATE_THREADS) {
        float acc = 0.f;
#pragma unroll 4
        for (int k = 0; k < R; ++k) acc = fmaf(dh[k], w1[(size_t)k * C + c], acc);
        dpooled[b * C + c] = acc;
    }
}

// a parameter gradient's store: alpha * sum rounded to f32 first, then added to the target (so accumulate = target + the plain result)
MH_DEV void se_param_store(float* o, float sum, float alpha, int accumulate) {
    const float v = __fmul_rn(alpha, sum);
    *o = accumulate ? __fadd_rn(*o, v) : v;
}

// dw1[r][:] and db1[r], one workgroup per hidden unit r: the thread keeps w2[c][r] and its dw1 sums for its J <= 16 columns (c = tid + 256 j)
// in registers and walks the batch ascending -- dh = [hidden > 0] sum_c da[b][c] w2[c][r] (recomputed here: as much work as the gradient
// itself, and no workspace), then dw1[r][c] += dh * pooled[b][c].  Columns past C read a clamped address and carry w2 = 0 (branch-free
// loads: all 2 J of a batch row are in flight together).
template <int J>
__global__ __launch_bounds__(256) void se_gate_bwd_w1_kernel(const float* __restrict__ ds, const float* __restrict__ s,
                                                             const float* __restrict__ hidden, const float* __restrict__ pooled,
                                                             const float* __restrict__ w2, float* __restrict__ dw1, float* __restrict__ db1,
                                                             int B, int C, int R, float alpha, int accumulate) {
    __shared__ float red[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float wcol[J], acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = tid + 256 * j;
        const float w = w2[(size_t)min(c, C - 1) * R + r];
        wcol[j] = c < C ? w : 0.f;
        acc[j] = 0.f;
    }
    float bsum = 0.f;
    for (int b = 0; b < B; ++b) {
        const size_t row = (size_t)b * C;
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = min(tid + 256 * j, C - 1);
            part = fmaf(se_dgate(ds[row + c], s[row + c]), wcol[j], part);
        }
        part = wave_sum(part);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        const float tot = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
        const float dh = hidden[(size_t)b * R + r] > 0.f ? tot : 0.f;
        bsum += dh;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            acc[j] = fmaf(dh, pooled[row + min(tid + 256 * j, C - 1)], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = tid + 256 * j;
        if (c < C) se_param_store(dw1 + (size_t)r * C + c, acc[j], alpha, accumulate);
    }
    if (tid == 0) se_param_store(db1 + r, bsum, alpha, accumulate);
}

// dw2[c][r] = sum_b da[b][c] hidden[b][r] and db2[c] = sum_b da[b][c]: one thread per weight, the batch ascending
__global__ __launch_bounds__(256) void se_gate_bwd_w2_kernel(const float* __restrict__ ds, const float* __restrict__ s,
                                                             const float* __restrict__ hidden, float* __restrict__ dw2, float* __restrict__ db2,
                                                             int B, int C, int R, float alpha, int accumulate) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * R) return;
    const int c = idx / R, r = idx % R;
    float acc = 0.f, bsum = 0.f;
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
        const float d = se_dgate(ds[(size_t)b * C + c], s[(size_t)b * C + c]);
        acc = fmaf(d, hidden[(size_t)b * R + r], acc);
        bsum += d;
    }
    se_param_store(dw2 + idx, acc, alpha, accumulate);
    if (r == 0) se_param_store(db2 + c, bsum, alpha, accumulate);
}

// the shape rules: C a multiple of 8 in [8, 4096]; the gate: 1 <= R <= 256, B >= 1 (grid.x); the activation kernels: HW >= 1 with one image's
// HW * C / 8 chunks in 32 bits, 1 <= B <= 65535 (grid.y)
bool se_channels_ok(int C) { return C >= 8 && C <= SE_MAX_C && C % 8 == 0; }
bool se_shape_ok(int B, int HW, int C) {
    return B >= 1 && B <= 65535 && HW >= 1 && se_channels_ok(C) && (uint64_t)HW * (uint64_t)(C / 8) < (1ull << 31);
}
bool se_gate_shape_ok(int B, int C, int R) { return B >= 1 && se_channels_ok(C) && R >= 1 && R <= SE_MAX_R; }
bool se_misaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) != 0;
}
dim3 se_stream_grid(int B, uint32_t per) { return dim3((per + 255u) / 256u, B); }

}  // namespace

extern "C" int mh_se_gate_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden, float* s,
                              int B, int C, int R, mh_stream_t stream) {
    if (!pooled || !w1 || !b1 || !w2 || !b2 || !hidden || !s) return MH_EINVAL;
    if (!se_gate_shape_ok(B, C, R)) return MH_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(se_gate_hidden_kernel, dim3(B, (R + 3) / 4), dim3(256), 0, st, pooled, w1, b1, hidden, C, R);
    const dim3 grid(B, (C + 255) / 256);
    if (R % 4 == 0 && ((uintptr_t)w2 & 15) == 0) hipLaunchKernelGGL(se_gate_scale_kernel<true>, grid, dim3(256), 0, st, hidden, w2, b2, s, C, R);
    else hipLaunchKernelGGL(se_gate_scale_kernel<false>, grid, dim3(256), 0, st, hidden, w2, b2, s, C, R);
    return mh_launch_status();
}

extern "C" int mh_se_apply_fwd(const void* u, const float* s, const void* shortcut, void* y, int B, int HW, int C, mh_stream_t stream) {
    if (!u || !s || !shortcut || !y || se_misaligned(u, s, shortcut, y)) return MH_EINVAL;
    if (!se_shape_ok(B, HW, C)) return MH_ESHAPE;
    const uint32_t per = (uint32_t)HW * (uint32_t)(C / 8);
    hipLaunchKernelGGL(se_apply_fwd_kernel, se_stream_grid(B, per), dim3(256), 0, (hipStream_t)stream, (const h16*)u, s, (const h16*)shortcut,
                       (h16*)y, per, C);
    return mh_launch_status();
}

extern "C" int mh_se_apply_bwd_reduce(const void* dy, const void* y, const void* u, void* g, float* ds, int B, int HW, int C,
                                      mh_stream_t stream) {
    if (!dy || !y || !u || !g || !ds || se_misaligned(dy, y, u, g)) return MH_EINVAL;
    if (!se_shape_ok(B, HW, C)) return MH_ESHAPE;
    const dim3 grid((C + 63) / 64, B);
    // 16 waves a workgroup where there are few of them (layer1: 32 images x 4 column groups over 3136 rows), 4 where there are many
    if ((int64_t)B * ((C + 63) / 64) < 512 && HW > 128)
        hipLaunchKernelGGL(se_apply_bwd_reduce_kernel<1024>, grid, dim3(1024), 0, (hipStream_t)stream, (const h16*)dy, (const h16*)y,
                           (const h16*)u, (h16*)g, ds, HW, C);
    else
        hipLaunchKernelGGL(se_apply_bwd_reduce_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, (const h16*)dy, (const h16*)y,
                           (const h16*)u, (h16*)g, ds, HW, C);
    return mh_launch_status();
}

extern "C" int mh_se_gate_bwd(const float* ds, const float* s, const float* hidden, const float* pooled, const float* w1, const float* w2,
                              float* dpooled, float* dw1, float* db1, float* dw2, float* db2, int B, int C, int R, float alpha, int accumulate,
                              mh_stream_t stream) {
    if (!ds || !s || !hidden || !pooled || !w1 || !w2 || !dpooled || !dw1 || !db1 || !dw2 || !db2) return MH_EINVAL;
    if (!se_gate_shape_ok(B, C, R)) return MH_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(se_gate_bwd_dpooled_kernel, dim3(B), dim3(SE_GATE_THREADS), 0, st, ds, s, hidden, w1, w2, dpooled, C, R);
#define SE_W1(J_) hipLaunchKernelGGL(se_gate_bwd_w1_kernel<J_>, dim3(R), dim3(256), 0, st, ds, s, hidden, pooled, w2, dw1, db1, B, C, R, alpha, accumulate)
    if (C <= 256) SE_W1(1);
    else if (C <= 512) SE_W1(2);
    else if (C <= 1024) SE_W1(4);
    else if (C <= 2048) SE_W1(8);
    else SE_W1(16);
#undef SE_W1
    hipLaunchKernelGGL(se_gate_bwd_w2_kernel, dim3((C * R + 255) / 256), dim3(256), 0, st, ds, s, hidden, dw2, db2, B, C, R, alpha, accumulate);
    return mh_launch_status();
}

extern "C" int mh_se_apply_bwd(const void* g, const float* s, const float* dpooled, void* du, int B, int HW, int C, mh_stream_t stream) {
    if (!g || !s || !dpooled || !du || se_misaligned(g, s, dpooled, du)) return MH_EINVAL;
    if (!se_shape_ok(B, HW, C)) return MH_ESHAPE;
    const uint32_t per = (uint32_t)HW * (uint32_t)(C / 8);
    hipLaunchKernelGGL(se_apply_bwd_kernel, se_stream_grid(B, per), dim3(256), 0, (hipStream_t)stream, (const h16*)g, s, dpooled, (h16*)du, per, C,
                       (float)HW);
    return mh_launch_status();
}
