// The body of the depthwise tile kernel, included by dwconv.hip once per direction (the forward kernel's text is exactly what it was:
// its register allocation and load schedule are pinned by tools/isa_bands.json).
//   DW_DGRAD 0: y = bias + conv(x, wt)                      (x, wt, bias, y)
//   DW_DGRAD 1: dx = addend + conv(dy, wt taps reversed)    (x = dy, wt, addend, y = dx): for an odd k with padding k/2 the input
//               gradient is this same convolution over dy with tap (k-1-ky, k-1-kx) -- same halo tile in LDS, same thread mapping.
// In scope: x, wt, y, H, W, C, CB, tiles_x, template <int T, int KS>.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int HT = T + KS - 1, PAD = KS / 2;
    const int groups = CB / 8;                       // 8-channel groups of this chunk
    const int tid = threadIdx.x, nthr = groups * T;  // blockDim.x == nthr
    const int b = blockIdx.z, c_chunk = blockIdx.y * CB;
    const int ty0 = (blockIdx.x / tiles_x) * T, tx0 = (blockIdx.x % tiles_x) * T;
    const h16* xb = x + (size_t)b * H * W * C + c_chunk;

    for (int q = tid; q < HT * HT * groups; q += nthr) {
        const int pix = q / groups, cg = q - pix * groups;
        const int iy = ty0 - PAD + pix / HT, ix = tx0 - PAD + pix % HT;
        i32x4 v = {0, 0, 0, 0};
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const i32x4*)(xb + ((size_t)iy * W + ix) * C + cg * 8);
        *(i32x4*)(smem + ((size_t)pix * CB + cg * 8) * 2) = v;
    }
    __syncthreads();

    const int g = tid % groups, r = tid / groups;    // channel group, output row of the tile
    const int c0 = c_chunk + g * 8;
    float acc[T][8];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < KS; ++ky) {
        Pack8 in[HT];
#pragma unroll
        for (int i = 0; i < HT; ++i) in[i].v = *(const i32x4*)(smem + ((size_t)((r + ky) * HT + i) * CB + g * 8) * 2);
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
#if DW_DGRAD
            const float* wp = wt + (size_t)((KS - 1 - ky) * KS + (KS - 1 - kx)) * C + c0;      // the taps in reverse
#else
            const float* wp = wt + (size_t)(ky * KS + kx) * C + c0;
#endif
            const f32x4 w0 = *(const f32x4*)wp, w1 = *(const f32x4*)(wp + 4);
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[i][e] = fmaf(mh_bf2f(in[i + kx].e[e]), w0[e], acc[i][e]);
                    acc[i][4 + e] = fmaf(mh_bf2f(in[i + kx].e[4 + e]), w1[e], acc[i][4 + e]);
                }
        }
    }
#if !DW_DGRAD
    f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (bias) {
        b0 = *(const f32x4*)(bias + c0);
        b1 = *(const f32x4*)(bias + c0 + 4);
    }
#endif
    const int oy = ty0 + r;
    if (oy >= H) return;
    h16* yb = y + ((size_t)b * H + oy) * W * C + c0;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int ox = tx0 + i;
        if (ox >= W) break;
        Pack8 u;
#if DW_DGRAD
        if (addend) {      // the residual-branch gradient joins the f32 accumulator: one rounding
            Pack8 a;
            a.v = *(const i32x4*)(addend + (yb - y) + (size_t)ox * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) u.e[e] = mh_f2bf(acc[i][e] + mh_bf2f(a.e[e]));
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) u.e[e] = mh_f2bf(acc[i][e]);
        }
#else
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            u.e[e] = mh_f2bf(acc[i][e] + b0[e]);
            u.e[4 + e] = mh_f2bf(acc[i][4 + e] + b1[e]);
        }
#endif
        *(i32x4*)(yb + (size_t)ox * C) = u.v;
    }
