// Autoregressive decode kernels of the BLIP caption decoder (blip.BlipCaptioner): one new token per row and step.
//
//   mh_attn_decode   one query per (row, head) against T cached keys / values (head dim 64, scale 1/8, online softmax in f32);
//                    the self-attention form first stores this step's k / v into cache slot t (t read on the device)
//   mh_decode_embed  LayerNorm(word[id] + pos[t]) for one token per row (id and t read on the device)
//   mh_greedy_step   row argmax of the LM head's f32 logits + the greedy bookkeeping of transformers' generate
//
// Every state that changes from step to step (t, the input ids, the finished flags) lives in device memory, so one step is
// captured once as a hipGraph and replayed per token.  Every sum runs in a fixed order: results are bit-identical run to run.
//
// Why no MFMA in mh_attn_decode: with one query row per (row, head) the score product is a matrix-VECTOR product (64 MACs per
// 128-byte key row, the same for P.V), i.e. 1 FLOP per byte read.  The kernel is bound by reading the cache (cross-attention over
// 577 image tokens: 148 KB per (row, head)); MFMA would pad the query to 16 rows and compute 15 rows of nothing.  Lanes are grouped
// in eights instead: each group owns one key at a time and each lane a 16-byte slice (8 of the 64 dims) of its key and value rows.
#include "common.h"

namespace {

constexpr int DEC_THREADS = 256;
constexpr int DEC_GROUPS = DEC_THREADS / 8;     // keys in flight per workgroup and unrolled step
constexpr int DEC_WS = 66;                      // workspace floats per (row, head, split): m, l, acc[64]
constexpr float DEC_SCALE_LOG2 = 0.125f * 1.44269504088896341f;      // 1/sqrt(64), in the exp2 domain

struct DecodeArgs {
    const h16* q;          // q of (b, h) at q + b*ldq + h*64
    h16* k;                // k of (b, h, j) at k + b*ld_b + j*ld_t + h*64 (v likewise)
    h16* v;
    const h16* kv_new;     // self form: this step's k of (b, h) at kv_new + b*ld_new + h*64, its v H*64 further
    const int32_t* t_dev;  // self form: the slot of this step (keys 0..t attend; t >= T: no store, keys 0..T-1); NULL: T keys
    h16* out;              // out of (b, h) at out + b*ldo + h*64
    float* ws;             // nsplit > 1: [B*H][nsplit][DEC_WS]
    int64_t ld_b;
    int ldq, ld_t, ld_new, ldo, T, H, nsplit, chunk;
};

MH_DEV float sum8(float x, unsigned lane) {      // sum over the 8 lanes of a group (lanes 8g .. 8g+7)
    x += mh_xor_partner<1>(x, lane);
    x += mh_xor_partner<2>(x, lane);
    x += mh_xor_partner<4>(x, lane);
    return x;
}

MH_DEV void load8(const h16* p, float* f) {
    Pack8 u;
    u.v = *reinterpret_cast<const i32x4*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = mh_bf2f(u.e[i]);
}

__global__ void __launch_bounds__(DEC_THREADS) attn_decode_kernel(DecodeArgs a) {
    __shared__ float red[DEC_GROUPS][DEC_WS];
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, g = tid >> 3, l8 = tid & 7;
    const unsigned lane = mh_lane_id();
    const int t = a.t_dev ? a.t_dev[0] : -1;
    const int T = a.t_dev ? min(t + 1, a.T) : a.T;          // keys this step attends
    const h16* newk = a.kv_new ? a.kv_new + (int64_t)b * a.ld_new + h * 64 : nullptr;
    const int64_t base = (int64_t)b * a.ld_b + h * 64;

    // self form: the split that owns slot t stores this step's k / v row there (the step itself reads them from kv_new)
    if (a.t_dev && t >= 0 && t < a.T && split == 0 && tid < 16) {
        const int off = (tid & 7) * 8;
        const i32x4 val = *reinterpret_cast<const i32x4*>(newk + (tid < 8 ? 0 : a.H * 64) + off);
        h16* dst = (tid < 8 ? a.k : a.v) + base + (int64_t)t * a.ld_t + off;
        *reinterpret_cast<i32x4*>(dst) = val;
    }

    float q[8];
    load8(a.q + (int64_t)b * a.ldq + h * 64 + l8 * 8, q);
    float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;

    const int j0 = split * a.chunk, j1 = min(T, j0 + a.chunk);
    for (int jb = j0 + g; jb < j1; jb += 2 * DEC_GROUPS) {
        // two keys per group and pass: their four 16-byte loads are issued together
        const int jj[2] = {jb, jb + DEC_GROUPS};
        float kf[2][8], vf[2][8], s[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = jj[u] < j1 ? jj[u] : jb;           // (a missing second key re-reads the first and is dropped below)
            const h16* kp = (j == t) ? newk : a.k + base + (int64_t)j * a.ld_t;
            const h16* vp = (j == t) ? newk + a.H * 64 : a.v + base + (int64_t)j * a.ld_t;
            load8(kp + l8 * 8, kf[u]);
            load8(vp + l8 * 8, vf[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) d += q[i] * kf[u][i];
            s[u] = sum8(d, lane) * DEC_SCALE_LOG2;
        }
        const bool two = jj[1] < j1;
        const float mn = fmaxf(m, two ? fmaxf(s[0], s[1]) : s[0]);
        const float c = __builtin_amdgcn_exp2f(m - mn);                 // m = -inf on the first key: 0
        const float p0 = __builtin_amdgcn_exp2f(s[0] - mn);
        const float p1 = two ? __builtin_amdgcn_exp2f(s[1] - mn) : 0.f;
        l = l * c + p0 + p1;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = acc[i] * c + p0 * vf[0][i] + p1 * vf[1][i];
        m = mn;
    }

    // the 32 groups' partials, combined in group order
    if (l8 == 0) {
        red[g][0] = m;
        red[g][1] = l;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[g][2 + l8 * 8 + i] = acc[i];
    __syncthreads();
    if (tid < 64) {
        float M = -INFINITY;
        for (int gg = 0; gg < DEC_GROUPS; ++gg) M = fmaxf(M, red[gg][0]);
        float L = 0.f, A = 0.f;
        if (M != -INFINITY) {
            for (int gg = 0; gg < DEC_GROUPS; ++gg) {
                const float mg = red[gg][0];
                if (mg == -INFINITY) continue;
                const float w = __builtin_amdgcn_exp2f(mg - M);
                L += red[gg][1] * w;
                A += red[gg][2 + tid] * w;
            }
        }
        if (a.nsplit > 1) {
            float* w = a.ws + ((int64_t)(b * a.H + h) * a.nsplit + split) * DEC_WS;
            if (tid == 0) {
                w[0] = M;
                w[1] = L;
            }
            w[2 + tid] = A;
        } else {
            a.out[(int64_t)b * a.ldo + h * 64 + tid] = mh_f2bf(L > 0.f ? A / L : 0.f);
        }
    }
}

// split partials of (b, h) -> out, in split order
__global__ void __launch_bounds__(64) attn_decode_combine_kernel(const float* ws, h16* out, int ldo, int H, int nsplit) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const float* w = ws + (int64_t)(b * H + h) * nsplit * DEC_WS;
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, w[s * DEC_WS]);
    float L = 0.f, A = 0.f;
    if (M != -INFINITY) {
        for (int s = 0; s < nsplit; ++s) {
            const float ms = w[s * DEC_WS];
            if (ms == -INFINITY) continue;
            const float e = __builtin_amdgcn_exp2f(ms - M);
            L += w[s * DEC_WS + 1] * e;
            A += w[s * DEC_WS + 2 + d] * e;
        }
    }
    out[(int64_t)b * ldo + h * 64 + d] = mh_f2bf(L > 0.f ? A / L : 0.f);
}

// block-wide sum in a fixed order (4 waves)
MH_DEV float block_sum256(float v, float* sh) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

constexpr int EMB_MAX_PER_THREAD = 8;     // D <= 2048

__global__ void __launch_bounds__(256) decode_embed_kernel(const int64_t* ids, const int32_t* t_dev, const float* word, const float* pos,
                                                          const float* gamma, const float* beta, h16* y, int D, int V, int P, float eps) {
    __shared__ float sh[4];
    const int b = blockIdx.x;
    int64_t id = ids[b];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    int t = t_dev[0];
    t = t < 0 ? 0 : (t >= P ? P - 1 : t);
    const float* wr = word + id * (int64_t)D;
    const float* pr = pos + (int64_t)t * D;
    float x[EMB_MAX_PER_THREAD];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < EMB_MAX_PER_THREAD; ++i) {
        const int d = threadIdx.x + i * 256;
        x[i] = d < D ? wr[d] + pr[d] : 0.f;
        s += x[i];
    }
    const float mean = block_sum256(s, sh) / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < EMB_MAX_PER_THREAD; ++i) {
        const int d = threadIdx.x + i * 256;
        const float c = d < D ? x[i] - mean : 0.f;
        q += c * c;
    }
    const float rstd = 1.0f / sqrtf(block_sum256(q, sh) / D + eps);
#pragma unroll
    for (int i = 0; i < EMB_MAX_PER_THREAD; ++i) {
        const int d = threadIdx.x + i * 256;
        if (d < D) y[(int64_t)b * D + d] = mh_f2bf((x[i] - mean) * rstd * gamma[d] + beta[d]);
    }
}

// (value, index) order of the argmax: larger value first, then the lower index (torch.argmax's first maximum); NaN ranks above
// every number, as in torch.argmax (a row holding a NaN yields its first NaN)
MH_DEV bool arg_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// state words: [0] t (the position this step consumed), [1] arrival counter (0 between launches), [2] rows finished,
// [3] output length once every row has finished (0 before)
__global__ void __launch_bounds__(256) greedy_step_kernel(const float* logits, int ldl, int V, int64_t* out_ids, int ld_out, int64_t* next_ids,
                                                          int32_t* finished, int32_t* state, int prompt_len, int64_t eos, int64_t pad) {
    __shared__ float shv[4];
    __shared__ int shi[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = state[0];
    const int col = t + 1;
    const bool fin = finished[b] != 0;
    const bool gen = col >= prompt_len && !fin;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (gen) {
        const float* row = logits + (int64_t)b * ldl;
        for (int c = tid * 4; c < V; c += 256 * 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c + i < V && arg_better(x[i], c + i, bv, bi)) {
                    bv = x[i];
                    bi = c + i;
                }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (arg_better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            shv[tid >> 6] = bv;
            shi[tid >> 6] = bi;
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (col < ld_out) {
            int64_t tok;
            if (col < prompt_len) {
                tok = out_ids[(int64_t)b * ld_out + col];         // still inside the prompt: its next token
            } else if (fin) {
                tok = pad;
            } else {
                for (int w = 1; w < 4; ++w)
                    if (arg_better(shv[w], shi[w], bv, bi)) {
                        bv = shv[w];
                        bi = shi[w];
                    }
                tok = bi < V ? bi : 0;
                if (tok == eos) {
                    finished[b] = 1;
                    const int nf = __hip_atomic_fetch_add(&state[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (nf == gridDim.x - 1) __hip_atomic_store(&state[3], col + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            out_ids[(int64_t)b * ld_out + col] = tok;
            next_ids[b] = tok;
        }
        // every workgroup has read t before it arrives (release); the last one to arrive advances t and re-arms the counter
        const int arrived = __hip_atomic_fetch_add(&state[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == gridDim.x - 1) {
            __hip_atomic_store(&state[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[0], t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" int mh_attn_decode(const void* q, int ldq, void* k, void* v, int64_t ld_b, int ld_t, const void* kv_new, int ld_new,
                              const int32_t* t_dev, int T, void* out, int ldo, float* workspace, int nsplit, int B, int H,
                              mh_stream_t stream) {
    if (!q || !k || !v || !out || (t_dev && !kv_new) || (nsplit > 1 && !workspace)) return MH_EINVAL;
    if (B < 1 || H < 1 || T < 1 || nsplit < 1 || nsplit > 64 || ldq % 8 || ld_t % 8 || ld_b % 8 || ld_new % 8 || ldo < H * 64)
        return MH_ESHAPE;
    DecodeArgs a;
    a.q = (const h16*)q;
    a.k = (h16*)k;
    a.v = (h16*)v;
    a.kv_new = (const h16*)kv_new;
    a.t_dev = t_dev;
    a.out = (h16*)out;
    a.ws = workspace;
    a.ld_b = ld_b;
    a.ldq = ldq; a.ld_t = ld_t; a.ld_new = ld_new; a.ldo = ldo;
    a.T = T; a.H = H; a.nsplit = nsplit;
    a.chunk = ((T + nsplit - 1) / nsplit + DEC_GROUPS - 1) / DEC_GROUPS * DEC_GROUPS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_decode_kernel, dim3(nsplit, H, B), dim3(DEC_THREADS), 0, s, a);
    if (nsplit > 1) hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(H, B), dim3(64), 0, s, (const float*)workspace, (h16*)out, ldo, H, nsplit);
    return mh_launch_status();
}

extern "C" int mh_decode_embed(const int64_t* ids, const int32_t* t_dev, const float* word, const float* pos, const float* gamma,
                               const float* beta, void* y, int B, int D, int V, int P, float eps, mh_stream_t stream) {
    if (!ids || !t_dev || !word || !pos || !gamma || !beta || !y) return MH_EINVAL;
    if (B < 1 || D < 1 || D > 256 * EMB_MAX_PER_THREAD || V < 1 || P < 1) return MH_ESHAPE;
    hipLaunchKernelGGL(decode_embed_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ids, t_dev, word, pos, gamma, beta, (h16*)y, D, V, P, eps);
    return mh_launch_status();
}

extern "C" int mh_greedy_step(const float* logits, int ldl, int V, int B, int64_t* out_ids, int ld_out, int64_t* next_ids,
                              int32_t* finished, int32_t* state, int prompt_len, int64_t eos_id, int64_t pad_id, mh_stream_t stream) {
    if (!logits || !out_ids || !next_ids || !finished || !state) return MH_EINVAL;
    if (B < 1 || V < 1 || ldl < V || ldl % 4 || prompt_len < 1 || ld_out <= prompt_len) return MH_ESHAPE;
    hipLaunchKernelGGL(greedy_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, out_ids, ld_out, next_ids, finished,
                       state, prompt_len, eos_id, pad_id);
    return mh_launch_status();
}
