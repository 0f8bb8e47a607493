// Autoregressive decode kernels of the BLIP caption decoder (blip.BlipCaptioner): one new token per row and step.
//
//   mh_attn_decode   one query per (row, head) against T cached keys / values (head dim 64, scale 1/8, online softmax in f32);
//                    the self-attention form first stores this step's k / v into cache slot t (t read on the device)
//   mh_decode_embed  LayerNorm(word[id] + pos[t]) for one token per row (id and t read on the device)
//   mh_greedy_step   row argmax of the LM head's f32 logits + the greedy bookkeeping of transformers' generate
//   mh_beam_step     beam search over the same logits (2 <= K <= 8 beams per image): log-softmax + the row's top 2K, then per image
//                    the ordered top 2K of K*V candidates and the running / finished bookkeeping of transformers' _beam_search
//   mh_greedy_step_processed / mh_beam_step_processed   the same two with transformers' repetition penalty, n-gram ban and minimum
//                    lengths applied inside the selection kernels (instantiations of their own: the plain ones are unchanged)
//   mh_sample_step   the greedy step with a temperature / top-k / top-p filtered multinomial draw in place of the argmax (with the
//                    processors first when any is set), one counter-hash uniform per (seed, row, column)
//
// Beams: the rows are [image][beam].  Cross-attention k / v stay one copy per image (kv_group rows share it).  The self-attention
// cache does not move when beams are re-ordered: an ancestry table src[row][position] names the physical cache row that holds the
// k / v of that position for the beam now living in `row`; mh_beam_step permutes the table, mh_attn_decode reads keys through it.
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
    const int32_t* src;    // beams: key j < t of row b lives in cache row src[b*ld_src + j] (NULL: in row b itself)
    int64_t ld_b;
    int ldq, ld_t, ld_new, ldo, T, H, nsplit, chunk, ld_src, kv_group;
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
    const int64_t base = (int64_t)(b / a.kv_group) * a.ld_b + h * 64;      // kv_group rows read one image's k / v
    const int32_t* srow = a.src ? a.src + (int64_t)b * a.ld_src : nullptr;
    const int last_row = (int)gridDim.z - 1;

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
        int64_t rb[2] = {base, base};
        if (srow) {                                          // both table entries of the trip are loaded before its keys
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = jj[u] < j1 ? jj[u] : jb;
                const int r = j == t ? b : srow[j];          // (slot t is this step's own: its entry is written by mh_beam_step)
                rb[u] = (int64_t)min(max(r, 0), last_row) * a.ld_b + h * 64;
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = jj[u] < j1 ? jj[u] : jb;           // (a missing second key re-reads the first and is dropped below)
            const h16* kp = (j == t) ? newk : a.k + rb[u] + (int64_t)j * a.ld_t;
            const h16* vp = (j == t) ? newk + a.H * 64 : a.v + rb[u] + (int64_t)j * a.ld_t;
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

// ---- logits processors (transformers' RepetitionPenalty, NoRepeatNGram, MinLength and MinNewTokensLength, in that order) ----------
// Both selection kernels stream a row of V logits with one workgroup.  The processed forms first stage the row's history (the L
// tokens so far, prompt included) into LDS and build two bitmaps of V bits there: `seen` (every history token: penalised once, however
// often it occurs) and `banned` (the token after every earlier occurrence of the last n - 1 tokens, and eos while the sequence is
// under either minimum length).  That costs O(L * n / 256) per thread and no pass over the vocabulary; the streaming loops then read
// one word of each bitmap per 16-byte chunk (a chunk starts at a multiple of 4, so its four bits share a word).
constexpr int PROC_MAX_V = MH_PROCESS_MAX_VOCAB;         // 2 bitmaps * 4 KB of static LDS
constexpr int PROC_MAX_HIST = MH_PROCESS_MAX_HISTORY;    // + 4 KB for the history

struct ProcArgs {
    float penalty;
    int ngram, min_length, min_new_tokens;
    int eos;      // -1: outside [0, V)
};

struct ProcLds {
    uint32_t seen[PROC_MAX_V / 32], banned[PROC_MAX_V / 32];
    int hist[PROC_MAX_HIST];
};

// hist: the row's tokens 0..L-1 (int64 for the greedy output rows, int32 for the beams' sequences), L <= PROC_MAX_HIST, V <= PROC_MAX_V.
// Called by the whole workgroup; the bitmaps are complete when it returns.  An id outside [0, V) has no logit and sets no bit.
template <typename Tok>
MH_DEV void proc_build(ProcLds& p, const Tok* hist, int L, int V, int prompt_len, const ProcArgs& a) {
    const int tid = threadIdx.x, n = a.ngram, eos = a.eos;
    for (int w = tid; w < (V + 31) / 32; w += 256) p.seen[w] = p.banned[w] = 0u;
    for (int j = tid; j < L; j += 256) p.hist[j] = (int)hist[j];
    __syncthreads();
    for (int j = tid; j < L; j += 256) {
        const int id = p.hist[j];
        if ((unsigned)id >= (unsigned)V) continue;
        atomicOr(&p.seen[id >> 5], 1u << (id & 31));
        if (n > 0 && j >= n - 1) {           // the window that ends at j: do its first n - 1 tokens equal the last n - 1 of the row?
            bool match = true;
            for (int k = 1; k < n && match; ++k) match = p.hist[j - k] == p.hist[L - k];
            if (match) atomicOr(&p.banned[id >> 5], 1u << (id & 31));
        }
    }
    // (L is read from the device step counter by the caller: the launch is replayed from a graph)
    if (tid == 0 && (unsigned)eos < (unsigned)V && (L < a.min_length || L - prompt_len < a.min_new_tokens))
        atomicOr(&p.banned[eos >> 5], 1u << (eos & 31));
    __syncthreads();
}

// one value: penalise (s < 0 ? s * p : s / p, each one correctly rounded f32 operation), then ban
MH_DEV float proc_apply(float v, uint32_t seen, uint32_t banned, int i, float penalty) {
    if ((seen >> i) & 1u) v = v < 0.f ? __fmul_rn(v, penalty) : __fdiv_rn(v, penalty);
    return ((banned >> i) & 1u) ? -INFINITY : v;
}

// state words: [0] t (the position this step consumed), [1] arrival counter (0 between launches), [2] rows finished,
// [3] output length once every row has finished (0 before)
template <bool PROC>
MH_DEV void greedy_step_body(const float* logits, int ldl, int V, int64_t* out_ids, int ld_out, int64_t* next_ids, int32_t* finished,
                             int32_t* state, int prompt_len, int64_t eos, int64_t pad, const ProcArgs& pa, ProcLds* pl) {
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
        if constexpr (PROC) proc_build(*pl, out_ids + (int64_t)b * ld_out, min(col, ld_out), V, prompt_len, pa);
        for (int c = tid * 4; c < V; c += 256 * 4) {
            f32x4 x = *reinterpret_cast<const f32x4*>(row + c);
            if constexpr (PROC) {
                const uint32_t sw = pl->seen[c >> 5] >> (c & 31), bw = pl->banned[c >> 5] >> (c & 31);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = proc_apply(x[i], sw, bw, i, pa.penalty);
            }
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

__global__ void __launch_bounds__(256) greedy_step_kernel(const float* logits, int ldl, int V, int64_t* out_ids, int ld_out, int64_t* next_ids,
                                                          int32_t* finished, int32_t* state, int prompt_len, int64_t eos, int64_t pad) {
    greedy_step_body<false>(logits, ldl, V, out_ids, ld_out, next_ids, finished, state, prompt_len, eos, pad, ProcArgs{}, nullptr);
}

__global__ void __launch_bounds__(256) greedy_step_processed_kernel(const float* logits, int ldl, int V, int64_t* out_ids, int ld_out,
                                                                    int64_t* next_ids, int32_t* finished, int32_t* state, int prompt_len,
                                                                    int64_t eos, int64_t pad, ProcArgs pa) {
    __shared__ ProcLds pl;
    greedy_step_body<true>(logits, ldl, V, out_ids, ld_out, next_ids, finished, state, prompt_len, eos, pad, pa, &pl);
}

// ---- sampling (transformers' TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, then one multinomial draw) ---------------
// One workgroup per row, the greedy step's contract.  Wave w owns the contiguous quarter [w * Q, (w + 1) * Q) of the row and reads it
// 256 values per trip (lane l the four values at 4 l of the trip: coalesced 16-byte loads), so the index order is (wave, trip, lane,
// element) and every prefix sum below follows it.  The row is re-read from L2 in each pass (122 KB at V = 30524), and every pass
// recomputes v = canon(fdiv_rn(proc_apply(x), temperature)) with the same correctly rounded operations (canon: -0 becomes +0, so that
// equal values have equal keys).  Passes:
//   1. m = the row's maximum and greedy's arg_better winner.  m not finite (a NaN, +inf, or an all -inf row): Z would not be a positive
//      finite number, and the winner is the token.  Past this point every v is finite or -inf and e = expf(v - m) lies in [0, 1].
//   2. top-k (0 < top_k < V): radix select of the k-th largest order-preserving uint key, 8 bits per pass: 256 integer counts in LDS.
//      Kept: key >= that key, ties at the threshold included (TopKLogitsWarper removes `scores < kth`).
//   3. top-p (top_p < 1): radix select by mass over the top-k survivors.  The masses are integers, e * 2^40 truncated into uint64, so a
//      bin's mass is an exact, order-independent sum of LDS integer atomics (no floating-point atomic anywhere).  A value is kept iff
//      the survivors' mass strictly above it is < top_p * Z, compared in double.  Equal values share a key, so equal values that
//      straddle the boundary are all kept (torch.sort leaves that choice open).  Truncation loses < 2^-40 per value, < 2^-25 of Z
//      over 32768 values (Z >= 2^40 in these units: the maximum contributes e = 1).
//   4. the draw, in f32: u = (h >> 8) * 2^-24, target = u * Z_kept, and the token is the first kept index whose inclusive prefix mass
//      exceeds the target; if rounding leaves none, the last kept index with a finite value.  Summation chains: a lane's four values
//      (3 additions), the trip's scan or sum across the wave's 64 lanes (6), the wave's running total over its trips (at most 32 at
//      V = 32768), the three earlier waves (3) and the two additions that join these parts: at most 46 f32 additions on any term's
//      way into any mass, inside the 256 the contract allows, so every mass is within 256 * 2^-24 = 2^-16 of its exact value
//      relative to Z.  All of it runs in a fixed order: the same logits, settings and seed give the same token on every run.
// Histogram bins are kept in SMP_COPIES copies selected by lane & 7 (logits share their high key bits, so the first pass of a select
// sends most values to a few bins; the copies cut that LDS conflict by eight) and summed, as integers, when a pass ends.
constexpr int SMP_COPIES = 8;
constexpr float SMP_FX = 1099511627776.0f;      // 2^40

struct SampleArgs {
    float temperature, top_p;
    int top_k;
};

struct SampleLds {
    unsigned long long mass[256 * SMP_COPIES];
    uint32_t cnt[256 * SMP_COPIES];
    unsigned long long w64[4], pick_above;
    uint32_t w32[4], pick_bin, pick_need;
    float wf[4];
    int wi[4], wj[4];
};

MH_DEV uint32_t sample_key(float x) {            // larger float <=> larger key (x is finite, +-inf or canonical zero)
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// uniform of (row, col) under the seed words: (h >> 8) * 2^-24 in [0, 1)
MH_DEV float sample_uniform(const uint32_t* rng, uint32_t row, uint32_t col) {
    uint32_t h = mh_hash32(rng[0] ^ 0x9E3779B9u);
    h = mh_hash32(h + rng[1]);
    h = mh_hash32(h + row);
    h = mh_hash32(h + col);
    return (float)(h >> 8) * 5.9604644775390625e-08f;
}

// The raw logits of SMP_AHEAD consecutive trips of a lane (columns c0 + 256 u .. + 3), loaded together: a wave has one quarter of
// the row to itself, so a pass is bound by the latency of its loads unless several are in flight.  A trip at or past `end` reads
// column `safe` instead (a multiple of 4 below `end`: an address inside the row; the caller drops the values).
constexpr int SMP_AHEAD = 4;

MH_DEV void sample_fetch(const float* row, int c0, int end, int safe, f32x4 (&raw)[SMP_AHEAD]) {
#pragma unroll
    for (int u = 0; u < SMP_AHEAD; ++u) {
        const int c = c0 + 256 * u;
        raw[u] = *reinterpret_cast<const f32x4*>(row + (c < end ? c : safe));
    }
}

// the four processed, tempered values of the raw logits x at columns c .. c + 3 (c a multiple of 4 below V)
template <bool PROC>
MH_DEV void sample_load4(f32x4 x, int c, const ProcLds* pl, const ProcArgs& pa, float temperature, float (&v)[4]) {
    if constexpr (PROC) {
        const uint32_t sw = pl->seen[c >> 5] >> (c & 31), bw = pl->banned[c >> 5] >> (c & 31);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = proc_apply(x[i], sw, bw, i, pa.penalty);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float y = temperature != 1.f ? __fdiv_rn(x[i], temperature) : x[i];
        v[i] = y == 0.f ? 0.f : y;
    }
}

template <typename T>
MH_DEV T wave_incl_scan(T v, unsigned lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T n = __shfl_up(v, o, 64);
        if (lane >= (unsigned)o) v += n;
    }
    return v;
}

// inclusive scan over the 256 threads in thread order (integers: exact), and the total
template <typename T>
MH_DEV T block_incl_scan(T v, T* sh, T& total) {
    const int w = threadIdx.x >> 6;
    const unsigned lane = threadIdx.x & 63;
    v = wave_incl_scan(v, lane);
    __syncthreads();
    if (lane == 63) sh[w] = v;
    __syncthreads();
    T off = 0;
    for (int i = 0; i < w; ++i) off += sh[i];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    return v + off;
}

// One histogram pass: the values whose key agrees with pfx above bit shift + 8 and is >= floor_key, binned by key bits
// shift .. shift + 7.  MASS: the bins receive e * 2^40, else 1.  Complete (and synchronised) when it returns.
template <bool PROC, bool MASS>
MH_DEV void sample_hist(SampleLds& L, const float* row, int V, int Q, const ProcLds* pl, const ProcArgs& pa, float temperature, float m,
                        uint32_t pfx, int shift, uint32_t floor_key) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int i = tid; i < 256 * SMP_COPIES; i += 256) {
        if constexpr (MASS) L.mass[i] = 0ull;
        else L.cnt[i] = 0u;
    }
    __syncthreads();
    const int end = min((w + 1) * Q, V);
    for (int c0 = w * Q + lane * 4; c0 < end; c0 += 256 * SMP_AHEAD) {
        f32x4 raw[SMP_AHEAD];
        sample_fetch(row, c0, end, c0, raw);
#pragma unroll
        for (int u = 0; u < SMP_AHEAD; ++u) {
            const int c = c0 + 256 * u;
            if (c >= end) break;
            float v[4];
            sample_load4<PROC>(raw[u], c, pl, pa, temperature, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t key = sample_key(v[i]);
                if (c + i < V && key >= floor_key && (shift == 24 || ((key ^ pfx) >> (shift + 8)) == 0u)) {
                    const int slot = (int)((key >> shift) & 255u) * SMP_COPIES + (lane & (SMP_COPIES - 1));
                    if constexpr (MASS) atomicAdd(&L.mass[slot], (unsigned long long)(expf(v[i] - m) * SMP_FX));
                    else atomicAdd(&L.cnt[slot], 1u);
                }
            }
        }
    }
    __syncthreads();
}

template <bool PROC>
MH_DEV void sample_step_body(const float* logits, int ldl, int V, int64_t* out_ids, int ld_out, int64_t* next_ids, int32_t* finished,
                             int32_t* state, int prompt_len, int64_t eos, int64_t pad, const SampleArgs& sa, const uint32_t* rng,
                             float* u_out, const ProcArgs& pa, ProcLds* pl, SampleLds& L) {
    const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
    const unsigned lane = tid & 63;
    const int t = state[0];
    const int col = t + 1;
    const bool fin = finished[b] != 0;
    const bool gen = col >= prompt_len && !fin;
    const float u = sample_uniform(rng, (uint32_t)b, (uint32_t)col);
    int tok_s = 0;
    if (gen) {
        const float* row = logits + (int64_t)b * ldl;
        const float T = sa.temperature;
        const int Q = ((V + 3) / 4 + 255) & ~255;              // a wave's span: whole trips of 256
        const int base0 = w * Q, end = min((w + 1) * Q, V);    // (wave-uniform)
        if constexpr (PROC) proc_build(*pl, out_ids + (int64_t)b * ld_out, min(col, ld_out), V, prompt_len, pa);

        // 1. maximum and greedy's winner
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int c0 = base0 + (int)lane * 4; c0 < end; c0 += 256 * SMP_AHEAD) {
            f32x4 raw[SMP_AHEAD];
            sample_fetch(row, c0, end, c0, raw);
#pragma unroll
            for (int u = 0; u < SMP_AHEAD; ++u) {
                const int c = c0 + 256 * u;
                if (c >= end) break;
                float v[4];
                sample_load4<PROC>(raw[u], c, pl, pa, T, v);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c + i < V && arg_better(v[i], c + i, bv, bi)) {
                        bv = v[i];
                        bi = c + i;
                    }
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
        if (lane == 0) {
            L.wf[w] = bv;
            L.wi[w] = bi;
        }
        __syncthreads();
        bv = L.wf[0], bi = L.wi[0];
        for (int ww = 1; ww < 4; ++ww)
            if (arg_better(L.wf[ww], L.wi[ww], bv, bi)) {
                bv = L.wf[ww];
                bi = L.wi[ww];
            }
        const float m = bv;
        tok_s = bi < V ? bi : 0;
        __syncthreads();                                         // (wf / wi are written again below)

        if (fabsf(m) <= 3.402823466e38f) {                       // finite (uniform over the workgroup: every thread holds the same m)
            // 2. top-k: the k-th largest key
            uint32_t kkey = 0u;
            if (sa.top_k > 0 && sa.top_k < V) {
                uint32_t pfx = 0u, need = (uint32_t)sa.top_k;
                for (int shift = 24; shift >= 0; shift -= 8) {
                    sample_hist<PROC, false>(L, row, V, Q, pl, pa, T, m, pfx, shift, 0u);
                    const int bin = 255 - tid;                   // thread order = descending bins
                    uint32_t cb = 0u;
#pragma unroll
                    for (int i = 0; i < SMP_COPIES; ++i) cb += L.cnt[bin * SMP_COPIES + i];
                    uint32_t total;
                    const uint32_t incl = block_incl_scan(cb, L.w32, total), excl = incl - cb;
                    if (excl < need && need <= incl) {
                        L.pick_bin = (uint32_t)bin;
                        L.pick_need = need - excl;
                    }
                    __syncthreads();
                    pfx |= (L.pick_bin & 255u) << shift;
                    need = L.pick_need;
                }
                kkey = pfx;
            }
            // 3. top-p: the lowest key whose mass strictly above is < top_p * Z
            uint32_t tkey = kkey;
            if (sa.top_p < 1.f) {
                uint32_t pfx = 0u;
                unsigned long long above = 0ull;
                double pz = 0.0;
                for (int shift = 24; shift >= 0; shift -= 8) {
                    sample_hist<PROC, true>(L, row, V, Q, pl, pa, T, m, pfx, shift, kkey);
                    const int bin = 255 - tid;
                    unsigned long long mb = 0ull;
#pragma unroll
                    for (int i = 0; i < SMP_COPIES; ++i) mb += L.mass[bin * SMP_COPIES + i];
                    unsigned long long total;
                    const unsigned long long incl = block_incl_scan(mb, L.w64, total) + above, excl = incl - mb;
                    if (shift == 24) pz = (double)sa.top_p * (double)total;
                    // the bin in which the mass from the top first reaches top_p * Z: it holds the threshold
                    if ((double)excl < pz && !((double)incl < pz)) {
                        L.pick_bin = (uint32_t)bin;
                        L.pick_above = excl;
                    }
                    __syncthreads();
                    pfx |= (L.pick_bin & 255u) << shift;
                    above = L.pick_above;
                }
                tkey = pfx;
            }
            // 4. the draw.  First the kept mass: per trip the wave's tree sum, accumulated trip by trip, then the four waves in order
            float run = 0.f;
            for (int cb0 = base0; cb0 < end; cb0 += 256 * SMP_AHEAD) {
                f32x4 raw[SMP_AHEAD];
                sample_fetch(row, cb0 + (int)lane * 4, end, base0, raw);
#pragma unroll
                for (int u = 0; u < SMP_AHEAD; ++u) {
                    const int cb = cb0 + 256 * u;                // (wave-uniform trips: the shuffles below need every lane)
                    if (cb >= end) break;
                    const int c = cb + (int)lane * 4;
                    float e[4] = {0.f, 0.f, 0.f, 0.f};
                    if (c < end) {
                        float v[4];
                        sample_load4<PROC>(raw[u], c, pl, pa, T, v);
#pragma unroll
                        for (int i = 0; i < 4; ++i) e[i] = (c + i < V && sample_key(v[i]) >= tkey) ? expf(v[i] - m) : 0.f;
                    }
                    run += wave_sum(((e[0] + e[1]) + e[2]) + e[3]);
                }
            }
            if (lane == 0) L.wf[w] = run;
            __syncthreads();
            const float woff = w == 0 ? 0.f : (w == 1 ? L.wf[0] : (w == 2 ? L.wf[0] + L.wf[1] : (L.wf[0] + L.wf[1]) + L.wf[2]));
            const float Z = ((L.wf[0] + L.wf[1]) + L.wf[2]) + L.wf[3];
            if (Z > 0.f && Z < INFINITY) {
                const float target = __fmul_rn(u, Z);
                // then the same walk again: inclusive prefix of a value = (waves before + trips before) + (lanes before + the lane's own)
                int first = 0x7fffffff, last = -1;
                run = 0.f;
                for (int cb0 = base0; cb0 < end; cb0 += 256 * SMP_AHEAD) {
                    f32x4 raw[SMP_AHEAD];
                    sample_fetch(row, cb0 + (int)lane * 4, end, base0, raw);
#pragma unroll
                    for (int u = 0; u < SMP_AHEAD; ++u) {
                        const int cb = cb0 + 256 * u;
                        if (cb >= end) break;
                        const int c = cb + (int)lane * 4;
                        float e[4] = {0.f, 0.f, 0.f, 0.f};
                        bool kept[4] = {false, false, false, false};
                        if (c < end) {
                            float v[4];
                            sample_load4<PROC>(raw[u], c, pl, pa, T, v);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                kept[i] = c + i < V && sample_key(v[i]) >= tkey && v[i] != -INFINITY;
                                e[i] = kept[i] ? expf(v[i] - m) : 0.f;
                            }
                        }
                        const float s0 = e[0], s1 = s0 + e[1], s2 = s1 + e[2], s3 = s2 + e[3];
                        const float incl = wave_incl_scan(s3, lane);
                        float before = __shfl_up(incl, 1, 64);
                        if (lane == 0) before = 0.f;
                        const float base = woff + run;
                        const float pre[4] = {base + (before + s0), base + (before + s1), base + (before + s2), base + (before + s3)};
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (kept[i]) {
                                last = c + i;
                                if (pre[i] > target && first == 0x7fffffff) first = c + i;
                            }
                        run += wave_sum(s3);
                    }
                }
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    first = min(first, __shfl_xor(first, o, 64));
                    last = max(last, __shfl_xor(last, o, 64));
                }
                if (lane == 0) {
                    L.wi[w] = first;
                    L.wj[w] = last;
                }
                __syncthreads();
                first = min(min(L.wi[0], L.wi[1]), min(L.wi[2], L.wi[3]));
                last = max(max(L.wj[0], L.wj[1]), max(L.wj[2], L.wj[3]));
                if (first < V) tok_s = first;
                else if (last >= 0) tok_s = last;
            }
        }
    }
    if (tid == 0) {
        if (u_out) u_out[b] = u;
        if (col < ld_out) {
            int64_t tok;
            if (col < prompt_len) {
                tok = out_ids[(int64_t)b * ld_out + col];         // still inside the prompt: its next token
            } else if (fin) {
                tok = pad;
            } else {
                tok = tok_s;
                if (tok == eos) {
                    finished[b] = 1;
                    const int nf = __hip_atomic_fetch_add(&state[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (nf == gridDim.x - 1) __hip_atomic_store(&state[3], col + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            out_ids[(int64_t)b * ld_out + col] = tok;
            next_ids[b] = tok;
        }
        // the greedy step's arrival protocol: the last workgroup to arrive advances t and re-arms the counter
        const int arrived = __hip_atomic_fetch_add(&state[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == gridDim.x - 1) {
            __hip_atomic_store(&state[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[0], t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ void __launch_bounds__(256) sample_step_kernel(const float* logits, int ldl, int V, int64_t* out_ids, int ld_out, int64_t* next_ids,
                                                          int32_t* finished, int32_t* state, int prompt_len, int64_t eos, int64_t pad,
                                                          SampleArgs sa, const uint32_t* rng, float* u_out) {
    __shared__ SampleLds L;
    sample_step_body<false>(logits, ldl, V, out_ids, ld_out, next_ids, finished, state, prompt_len, eos, pad, sa, rng, u_out, ProcArgs{},
                            nullptr, L);
}

__global__ void __launch_bounds__(256) sample_step_processed_kernel(const float* logits, int ldl, int V, int64_t* out_ids, int ld_out,
                                                                    int64_t* next_ids, int32_t* finished, int32_t* state, int prompt_len,
                                                                    int64_t eos, int64_t pad, SampleArgs sa, const uint32_t* rng,
                                                                    float* u_out, ProcArgs pa) {
    __shared__ SampleLds L;
    __shared__ ProcLds pl;
    sample_step_body<true>(logits, ldl, V, out_ids, ld_out, next_ids, finished, state, prompt_len, eos, pad, sa, rng, u_out, pa, &pl, L);
}

// ---- beam search ------------------------------------------------------------------------------------------------------------------
// One order everywhere: the larger f32 value first, then the lower index (the flat candidate index beam * V + token in the image's
// top 2K, the position in the later selections).  torch.topk leaves ties open; this is the rule they get here.
constexpr int BEAM_MAX = 8;
constexpr float BEAM_NEG = -1.0e9f;

MH_DEV bool beam_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

MH_DEV void lse_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    s = s * (m == M ? 1.f : expf(m - M)) + os * (om == M ? 1.f : expf(om - M));
    m = M;
}

// One workgroup per beam row: the row's log-sum-exp (f32, fixed order) and its own top N = 2K accumulated log-probabilities
// ((x - max) - log(sum)) + score, the oracle's f32 operations in its order.  The image's top 2K is a subset of the union of these.
// The second pass re-reads the row (122 KB at V = 30524, from L2) because the order is taken on the rounded accumulated value: two
// logits that round to one value tie, and the tie goes to the lower index.
// PROC: the processors act on the log-probability (x - max) - log(sum), before the score is added; the log-sum-exp is taken over
// the unprocessed row.  The history is the row's own run_seq: mh_beam_step permuted it by parent at the end of the previous step.
template <int N, bool PROC>
MH_DEV void beam_row_body(const float* logits, int ldl, int V, const float* run_scores, const int32_t* state, int prompt_len, int cap,
                          float* cand_val, int32_t* cand_idx, const int32_t* run_seq, const ProcArgs& pa, ProcLds* pl) {
    __shared__ float shm[4], shs[4];
    __shared__ int shi[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int col = state[0] + 1;
    if (col < prompt_len || col >= cap) return;           // inside the prompt, or past the end: no candidates are needed
    const float* row = logits + (int64_t)r * ldl;
    if constexpr (PROC) proc_build(*pl, run_seq + (int64_t)r * cap, col, V, prompt_len, pa);
    float m = -INFINITY, s = 0.f;
    for (int c = tid * 4; c < V; c += 256 * 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (c + i < V && x[i] != -INFINITY) {
                if (x[i] > m) {
                    s = s * expf(m - x[i]) + 1.f;
                    m = x[i];
                } else {
                    s += expf(x[i] - m);
                }
            }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
        lse_merge(m, s, om, os);
    }
    if ((tid & 63) == 0) {
        shm[tid >> 6] = m;
        shs[tid >> 6] = s;
    }
    __syncthreads();
    m = shm[0], s = shs[0];
    for (int w = 1; w < 4; ++w) lse_merge(m, s, shm[w], shs[w]);
    const float lse = logf(s), score = run_scores[r];

    float lv[N];
    int li[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        lv[n] = -INFINITY;
        li[n] = 0x7fffffff;
    }
    for (int c = tid * 4; c < V; c += 256 * 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + c);
        f32x4 lp;
#pragma unroll
        for (int i = 0; i < 4; ++i) lp[i] = (x[i] - m) - lse;
        if constexpr (PROC) {
            const uint32_t sw = pl->seen[c >> 5] >> (c & 31), bw = pl->banned[c >> 5] >> (c & 31);
#pragma unroll
            for (int i = 0; i < 4; ++i) lp[i] = proc_apply(lp[i], sw, bw, i, pa.penalty);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float f = lp[i] + score;
            if (c + i < V && beam_better(f, c + i, lv[N - 1], li[N - 1])) {
                lv[N - 1] = f;
                li[N - 1] = c + i;
#pragma unroll
                for (int n = N - 1; n > 0; --n)
                    if (beam_better(lv[n], li[n], lv[n - 1], li[n - 1])) {
                        const float tv = lv[n];
                        const int ti = li[n];
                        lv[n] = lv[n - 1], li[n] = li[n - 1];
                        lv[n - 1] = tv, li[n - 1] = ti;
                    }
            }
        }
    }
    // N rounds: the best entry of the workgroup that ranks after the previous round's winner
    float pv = INFINITY;
    int pi = -1;
    for (int round = 0; round < N; ++round) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int n = N - 1; n >= 0; --n)
            if (beam_better(pv, pi, lv[n], li[n])) {      // the list is sorted: the last hit from the back is the first from the front
                bv = lv[n];
                bi = li[n];
            }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (beam_better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        __syncthreads();
        if ((tid & 63) == 0) {
            shm[tid >> 6] = bv;
            shi[tid >> 6] = bi;
        }
        __syncthreads();
        bv = shm[0], bi = shi[0];
        for (int w = 1; w < 4; ++w)
            if (beam_better(shm[w], shi[w], bv, bi)) {
                bv = shm[w];
                bi = shi[w];
            }
        if (tid == 0) {
            cand_val[(int64_t)r * N + round] = bv;
            cand_idx[(int64_t)r * N + round] = bi;
        }
        pv = bv, pi = bi;
    }
}

template <int N>
__global__ void __launch_bounds__(256) beam_row_kernel(const float* logits, int ldl, int V, const float* run_scores, const int32_t* state,
                                                       int prompt_len, int cap, float* cand_val, int32_t* cand_idx) {
    beam_row_body<N, false>(logits, ldl, V, run_scores, state, prompt_len, cap, cand_val, cand_idx, nullptr, ProcArgs{}, nullptr);
}

template <int N>
__global__ void __launch_bounds__(256) beam_row_processed_kernel(const float* logits, int ldl, int V, const float* run_scores,
                                                                 const int32_t* state, int prompt_len, int cap, float* cand_val,
                                                                 int32_t* cand_idx, const int32_t* run_seq, ProcArgs pa) {
    __shared__ ProcLds pl;
    beam_row_body<N, true>(logits, ldl, V, run_scores, state, prompt_len, cap, cand_val, cand_idx, run_seq, pa, &pl);
}

MH_DEV int pick8(const int (&a)[BEAM_MAX], int p) {
    int v = a[0];
#pragma unroll
    for (int k = 1; k < BEAM_MAX; ++k) v = p == k ? a[k] : v;
    return v;
}

struct BeamArgs {
    MhBeamState s;
    int V, K, cap, prompt_len, early_stopping, eos;
    float length_penalty;
};

// One workgroup per image.  state words: [0] t, [1] arrival counter (0 between launches), [2] images closed in this step (0
// between launches), [3] 1 once no image can change its finished beams any more.
__global__ void __launch_bounds__(256) beam_image_kernel(BeamArgs a) {
    __shared__ float cv[2 * BEAM_MAX * BEAM_MAX], ov[2 * BEAM_MAX], ms[3 * BEAM_MAX], nrs[BEAM_MAX], nfs[BEAM_MAX];
    __shared__ int ci[2 * BEAM_MAX * BEAM_MAX], oi[2 * BEAM_MAX], cpar[2 * BEAM_MAX], ctok[2 * BEAM_MAX], hit[2 * BEAM_MAX], taken[3 * BEAM_MAX];
    __shared__ int rpar[BEAM_MAX], rtok[BEAM_MAX], ffrom[BEAM_MAX], mflag[3 * BEAM_MAX], mlen[3 * BEAM_MAX], nflag[BEAM_MAX], nlen[BEAM_MAX];
    const MhBeamState& S = a.s;
    const int b = blockIdx.x, tid = threadIdx.x, K = a.K, N = 2 * a.K, cap = a.cap, P = a.prompt_len;
    const int t = S.state[0], col = t + 1;
    const int r0 = b * K;
    bool closed = false;
    if (col < cap && col < P) {
        // inside the prompt: every beam takes the prompt's next token and stays where it is
        if (tid < K) {
            const int r = r0 + tid;
            S.next_ids[r] = S.run_seq[(int64_t)r * cap + col];
            S.parents[r] = tid;
            if (S.src && t >= 0) S.src[(int64_t)r * cap + t] = r;
        }
    } else if (col < cap) {
        const int n = K * N;
        if (tid < n) {
            const int beam = tid / N;
            cv[tid] = S.cand_val[(int64_t)r0 * N + tid];
            ci[tid] = beam * a.V + S.cand_idx[(int64_t)r0 * N + tid];
        }
        __syncthreads();
        if (tid < n) {                                    // rank by counting: the flat indices are distinct, so the ranks are too
            const float v = cv[tid];
            const int i = ci[tid];
            int rank = 0;
            for (int o = 0; o < n; ++o) rank += beam_better(cv[o], ci[o], v, i) ? 1 : 0;
            if (rank < N) {
                ov[rank] = v;
                oi[rank] = i;
            }
        }
        __syncthreads();
        if (tid == 0) {
            bool allhit = true;
            for (int j = 0; j < N; ++j) {
                cpar[j] = min(max(oi[j] / a.V, 0), K - 1);      // (in range whatever a row of NaNs left in the candidates)
                ctok[j] = min(max(oi[j] % a.V, 0), a.V - 1);
                hit[j] = (ctok[j] == a.eos || col + 1 >= cap) ? 1 : 0;
                allhit = allhit && hit[j];
            }
            // running beams: the best K of the 2K that do not stop
            for (int j = 0; j < N; ++j) {
                ms[j] = hit[j] ? ov[j] + BEAM_NEG : ov[j];
                taken[j] = 0;
            }
            for (int k = 0; k < K; ++k) {
                int best = -1;
                for (int j = 0; j < N; ++j)
                    if (!taken[j] && (best < 0 || ms[j] > ms[best])) best = j;
                taken[best] = 1;
                nrs[k] = ms[best];
                rpar[k] = cpar[best];
                rtok[k] = ctok[best];
            }
            // finished beams: the old K and the 2K candidates, merged; the best K stay
            const int glen = col + 1 - P;
            const float pen = (float)pow((double)glen, (double)a.length_penalty);
            bool allfin = true;
            for (int k = 0; k < K; ++k) allfin = allfin && S.fin_flags[r0 + k] != 0;
            const bool full = allfin && a.early_stopping == 1;
            bool heur = S.heur[b] != 0;
            for (int k = 0; k < K; ++k) {
                ms[k] = S.fin_scores[r0 + k];
                mflag[k] = S.fin_flags[r0 + k];
                mlen[k] = S.fin_len[r0 + k];
                taken[k] = 0;
            }
            for (int j = 0; j < N; ++j) {
                const bool did = hit[j] && j < K;
                float f = ov[j] / pen;
                if (full) f += BEAM_NEG;
                if (!heur) f += BEAM_NEG;
                if (!did) f += BEAM_NEG;
                ms[K + j] = f;
                mflag[K + j] = did ? 1 : 0;
                mlen[K + j] = glen;
                taken[K + j] = 0;
            }
            for (int k = 0; k < K; ++k) {
                int best = -1;
                for (int j = 0; j < K + N; ++j)
                    if (!taken[j] && (best < 0 || ms[j] > ms[best])) best = j;
                taken[best] = 1;
                ffrom[k] = best;
                nfs[k] = ms[best];
                nflag[k] = mflag[best];
                nlen[k] = mlen[best];
            }
            // can a running beam still beat the worst finished one?
            const int hyp = (a.early_stopping == 2 && a.length_penalty > 0.f) ? cap - P : glen;
            const float best_running = nrs[0] / (float)pow((double)hyp, (double)a.length_penalty);
            float worst = nfs[0];
            bool newall = true, any = false;
            for (int k = 0; k < K; ++k) {
                worst = fminf(worst, nfs[k]);
                newall = newall && nflag[k];
            }
            for (int k = 0; k < K; ++k) any = any || best_running > (nflag[k] ? worst : BEAM_NEG);
            heur = heur && any;
            for (int k = 0; k < K; ++k) {
                S.next_ids[r0 + k] = rtok[k];
                S.parents[r0 + k] = rpar[k];
                S.run_scores[r0 + k] = nrs[k];
                S.fin_scores[r0 + k] = nfs[k];
                S.fin_flags[r0 + k] = nflag[k];
                S.fin_len[r0 + k] = nlen[k];
            }
            S.heur[b] = heur ? 1 : 0;
            closed = !heur || (a.early_stopping == 1 && newall) || allhit;
        }
        __syncthreads();
        // the sequences and the cache's ancestry table follow the beams: one column per thread and pass, K values in registers
        for (int c = tid; c <= col; c += 256) {
            int orun[BEAM_MAX], ofin[BEAM_MAX], osrc[BEAM_MAX];
#pragma unroll
            for (int k = 0; k < BEAM_MAX; ++k) {
                const int64_t at = (int64_t)(r0 + (k < K ? k : 0)) * cap + c;
                orun[k] = S.run_seq[at];
                ofin[k] = S.fin_seq[at];
                osrc[k] = (S.src && c < t) ? S.src[at] : 0;
            }
#pragma unroll
            for (int k = 0; k < BEAM_MAX; ++k) {
                if (k >= K) break;
                const int64_t at = (int64_t)(r0 + k) * cap + c;
                S.run_seq[at] = c == col ? rtok[k] : pick8(orun, rpar[k]);
                const int from = ffrom[k];
                S.fin_seq[at] = from < K ? pick8(ofin, from) : (c == col ? ctok[from - K] : pick8(orun, cpar[from - K]));
                if (S.src && c <= t) S.src[at] = c == t ? r0 + rpar[k] : pick8(osrc, rpar[k]);
            }
        }
    }
    if (tid == 0) {
        if (closed) __hip_atomic_fetch_add(&S.state[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // every workgroup has read t and counted itself before it arrives; the last one to arrive advances t and re-arms the counters
        const int arrived = __hip_atomic_fetch_add(&S.state[1], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == (int)gridDim.x - 1) {
            const int nclosed = __hip_atomic_load(&S.state[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (nclosed == (int)gridDim.x) __hip_atomic_store(&S.state[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&S.state[2], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&S.state[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&S.state[0], t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" int mh_attn_decode_beams(const void* q, int ldq, void* k, void* v, int64_t ld_b, int ld_t, const void* kv_new, int ld_new,
                                    const int32_t* t_dev, int T, void* out, int ldo, float* workspace, int nsplit, int B, int H,
                                    int kv_group, const int32_t* src, int ld_src, mh_stream_t stream) {
    if (!q || !k || !v || !out || (t_dev && !kv_new) || (nsplit > 1 && !workspace) || (src && !t_dev)) return MH_EINVAL;
    if (B < 1 || H < 1 || T < 1 || nsplit < 1 || nsplit > 64 || ldq % 8 || ld_t % 8 || ld_b % 8 || ld_new % 8 || ldo < H * 64)
        return MH_ESHAPE;
    if (kv_group < 1 || B % kv_group || (t_dev && kv_group != 1) || (src && ld_src < T)) return MH_ESHAPE;
    DecodeArgs a;
    a.q = (const h16*)q;
    a.k = (h16*)k;
    a.v = (h16*)v;
    a.kv_new = (const h16*)kv_new;
    a.t_dev = t_dev;
    a.out = (h16*)out;
    a.ws = workspace;
    a.src = src;
    a.ld_src = ld_src;
    a.kv_group = kv_group;
    a.ld_b = ld_b;
    a.ldq = ldq; a.ld_t = ld_t; a.ld_new = ld_new; a.ldo = ldo;
    a.T = T; a.H = H; a.nsplit = nsplit;
    a.chunk = ((T + nsplit - 1) / nsplit + DEC_GROUPS - 1) / DEC_GROUPS * DEC_GROUPS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_decode_kernel, dim3(nsplit, H, B), dim3(DEC_THREADS), 0, s, a);
    if (nsplit > 1) hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(H, B), dim3(64), 0, s, (const float*)workspace, (h16*)out, ldo, H, nsplit);
    return mh_launch_status();
}

extern "C" int mh_attn_decode(const void* q, int ldq, void* k, void* v, int64_t ld_b, int ld_t, const void* kv_new, int ld_new,
                              const int32_t* t_dev, int T, void* out, int ldo, float* workspace, int nsplit, int B, int H,
                              mh_stream_t stream) {
    return mh_attn_decode_beams(q, ldq, k, v, ld_b, ld_t, kv_new, ld_new, t_dev, T, out, ldo, workspace, nsplit, B, H, 1, nullptr, 0, stream);
}

extern "C" int mh_decode_embed(const int64_t* ids, const int32_t* t_dev, const float* word, const float* pos, const float* gamma,
                               const float* beta, void* y, int B, int D, int V, int P, float eps, mh_stream_t stream) {
    if (!ids || !t_dev || !word || !pos || !gamma || !beta || !y) return MH_EINVAL;
    if (B < 1 || D < 1 || D > 256 * EMB_MAX_PER_THREAD || V < 1 || P < 1) return MH_ESHAPE;
    hipLaunchKernelGGL(decode_embed_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ids, t_dev, word, pos, gamma, beta, (h16*)y, D, V, P, eps);
    return mh_launch_status();
}

namespace {

const MhLogitsProcess PROC_NEUTRAL = {1.0f, 0, 0, 0};

// MH_EINVAL for settings outside their domain; *on: does any processor act?
int proc_settings(const MhLogitsProcess* p, int V, int64_t eos_id, ProcArgs* pa, bool* on) {
    if (!p) return MH_EINVAL;
    if (!(p->repetition_penalty > 0.f) || p->repetition_penalty > 3.0e38f || p->no_repeat_ngram_size < 0 || p->min_length < 0 ||
        p->min_new_tokens < 0)
        return MH_EINVAL;
    pa->penalty = p->repetition_penalty;
    pa->ngram = p->no_repeat_ngram_size;
    pa->min_length = p->min_length;
    pa->min_new_tokens = p->min_new_tokens;
    pa->eos = (eos_id >= 0 && eos_id < V) ? (int)eos_id : -1;
    *on = p->repetition_penalty != 1.0f || p->no_repeat_ngram_size > 0 || p->min_length > 0 || p->min_new_tokens > 0;
    return MH_OK;
}

}  // namespace

extern "C" int mh_greedy_step_processed(const float* logits, int ldl, int V, int B, int64_t* out_ids, int ld_out, int64_t* next_ids,
                                        int32_t* finished, int32_t* state, int prompt_len, int64_t eos_id, int64_t pad_id,
                                        const MhLogitsProcess* process, mh_stream_t stream) {
    if (!logits || !out_ids || !next_ids || !finished || !state) return MH_EINVAL;
    ProcArgs pa;
    bool on;
    if (const int st = proc_settings(process, V, eos_id, &pa, &on)) return st;
    if (B < 1 || V < 1 || ldl < V || ldl % 4 || prompt_len < 1 || ld_out <= prompt_len) return MH_ESHAPE;
    if (!on) {
        hipLaunchKernelGGL(greedy_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, out_ids, ld_out, next_ids,
                           finished, state, prompt_len, eos_id, pad_id);
        return mh_launch_status();
    }
    if (V > PROC_MAX_V || ld_out > PROC_MAX_HIST) return MH_ESHAPE;      // the bitmaps / the history do not fit their LDS
    hipLaunchKernelGGL(greedy_step_processed_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, out_ids, ld_out, next_ids,
                       finished, state, prompt_len, eos_id, pad_id, pa);
    return mh_launch_status();
}

extern "C" int mh_greedy_step(const float* logits, int ldl, int V, int B, int64_t* out_ids, int ld_out, int64_t* next_ids,
                              int32_t* finished, int32_t* state, int prompt_len, int64_t eos_id, int64_t pad_id, mh_stream_t stream) {
    return mh_greedy_step_processed(logits, ldl, V, B, out_ids, ld_out, next_ids, finished, state, prompt_len, eos_id, pad_id, &PROC_NEUTRAL,
                                    stream);
}

extern "C" int mh_sample_step(const float* logits, int ldl, int V, int B, int64_t* out_ids, int ld_out, int64_t* next_ids,
                              int32_t* finished, int32_t* state, int prompt_len, int64_t eos_id, int64_t pad_id, const MhSampling* sampling,
                              const uint32_t* rng, float* u_out, const MhLogitsProcess* process, mh_stream_t stream) {
    if (!logits || !out_ids || !next_ids || !finished || !state || !sampling || !rng) return MH_EINVAL;
    ProcArgs pa;
    bool on;
    if (const int st = proc_settings(process ? process : &PROC_NEUTRAL, V, eos_id, &pa, &on)) return st;
    if (B < 1 || V < 1 || ldl < V || ldl % 4 || prompt_len < 1 || ld_out <= prompt_len) return MH_ESHAPE;
    if (V > PROC_MAX_V || (on && ld_out > PROC_MAX_HIST)) return MH_ESHAPE;
    if (!(sampling->temperature > 0.f) || sampling->temperature > 3.0e38f || sampling->top_k < 0 || !(sampling->top_p > 0.f) ||
        sampling->top_p > 1.f)
        return MH_ESHAPE;
    SampleArgs sa;
    sa.temperature = sampling->temperature;
    sa.top_p = sampling->top_p;
    sa.top_k = sampling->top_k;
    if (on)
        hipLaunchKernelGGL(sample_step_processed_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, out_ids, ld_out,
                           next_ids, finished, state, prompt_len, eos_id, pad_id, sa, rng, u_out, pa);
    else
        hipLaunchKernelGGL(sample_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl, V, out_ids, ld_out, next_ids,
                           finished, state, prompt_len, eos_id, pad_id, sa, rng, u_out);
    return mh_launch_status();
}

extern "C" int mh_beam_step_processed(const float* logits, int ldl, int V, int B, int K, const MhBeamState* st, int cap, int prompt_len,
                                      float length_penalty, int early_stopping, int64_t eos_id, const MhLogitsProcess* process,
                                      mh_stream_t stream) {
    if (!logits || !st || !st->next_ids || !st->parents || !st->run_scores || !st->run_seq || !st->fin_seq || !st->fin_scores ||
        !st->fin_flags || !st->fin_len || !st->heur || !st->state || !st->cand_val || !st->cand_idx)
        return MH_EINVAL;
    ProcArgs pa;
    bool on;
    if (const int ps = proc_settings(process, V, eos_id, &pa, &on)) return ps;
    if (B < 1 || K < 2 || K > BEAM_MAX || V < 2 * K || (int64_t)K * V > 0x7fffffff || ldl < V || ldl % 4 || prompt_len < 1 ||
        cap <= prompt_len || early_stopping < 0 || early_stopping > 2 || (int64_t)B * K * cap > 0x7fffffff)
        return MH_ESHAPE;
    // processed: the bitmaps and the history fit their LDS, and the bans (at most one per history position, plus eos) leave every
    // row 2K finite candidates
    if (on && (V > PROC_MAX_V || cap > PROC_MAX_HIST || V < 2 * K + cap + 1)) return MH_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int R = B * K;
#define MH_BEAM_ROW(KK)                                                                                                               \
    case KK:                                                                                                                          \
        if (on)                                                                                                                       \
            hipLaunchKernelGGL(beam_row_processed_kernel<2 * KK>, dim3(R), dim3(256), 0, s, logits, ldl, V,                           \
                               (const float*)st->run_scores, (const int32_t*)st->state, prompt_len, cap, st->cand_val, st->cand_idx,  \
                               (const int32_t*)st->run_seq, pa);                                                                      \
        else                                                                                                                          \
            hipLaunchKernelGGL(beam_row_kernel<2 * KK>, dim3(R), dim3(256), 0, s, logits, ldl, V, (const float*)st->run_scores,       \
                               (const int32_t*)st->state, prompt_len, cap, st->cand_val, st->cand_idx);                               \
        break;
    switch (K) {
        MH_BEAM_ROW(2) MH_BEAM_ROW(3) MH_BEAM_ROW(4) MH_BEAM_ROW(5) MH_BEAM_ROW(6) MH_BEAM_ROW(7) MH_BEAM_ROW(8)
    }
#undef MH_BEAM_ROW
    BeamArgs a;
    a.s = *st;
    a.V = V; a.K = K; a.cap = cap; a.prompt_len = prompt_len; a.early_stopping = early_stopping; a.eos = (int)eos_id;
    a.length_penalty = length_penalty;
    hipLaunchKernelGGL(beam_image_kernel, dim3(B), dim3(256), 0, s, a);
    return mh_launch_status();
}

extern "C" int mh_beam_step(const float* logits, int ldl, int V, int B, int K, const MhBeamState* st, int cap, int prompt_len,
                            float length_penalty, int early_stopping, int64_t eos_id, mh_stream_t stream) {
    return mh_beam_step_processed(logits, ldl, V, B, K, st, cap, prompt_len, length_penalty, early_stopping, eos_id, &PROC_NEUTRAL, stream);
}
