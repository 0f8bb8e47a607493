// Linear C-SVC on the device: libsvm's SMO (Fan, Chen, Lin 2005, WSS2) for a batch of problems that share labels and Gram matrix
// and differ in their per-sample box bounds (C grids, class / sample weights, fold masks).  C ABI: include/memehip.h, "SVM".
//
// One workgroup of 1024 threads per problem, no grid-wide synchronisation.  Thread `tid` owns the samples t = s * 1024 + tid
// (s < SPT): their alpha and gradient G in float64 registers, K_tt, the label and the membership of I_up / I_low as bit masks.
// One iteration is
//   select i   per-thread scan, wave arg-max (DPP / permlane partners), one LDS slot per wave, barrier, 16-entry arg-max
//   row i      K[i][t] for the owned t (coalesced), second-order gain b^2 / a per t
//   select j   the same reduction
//   row j      K[j][t]; the two-variable update is computed redundantly by every thread from the slots' payload; G += ...
// so an iteration has two barriers (the LDS slots are double-buffered) and two dependent row loads.  Ties go to the lowest index.
// A launch runs at most `budget` iterations and leaves alpha, G and {status, iterations, gap, rho} in the caller's buffers; the
// next launch resumes from them.
#include <math.h>
#include <limits.h>
#include "common.h"

namespace {

constexpr int SVC_THREADS = 1024;
constexpr int SVC_WAVES = SVC_THREADS / 64;
constexpr double SVC_TAU = 1e-12;

struct Cand {
    double v;
    int idx;
};
// the larger value; among equals the lower index
MH_DEV Cand cand_best(Cand a, Cand b) { return (b.v > a.v || (b.v == a.v && b.idx < a.idx)) ? b : a; }
template <int O>
MH_DEV Cand cand_partner(Cand c, unsigned lane) {
    Cand r;
    r.v = mh_xor_partner_f64<O>(c.v, lane);
    r.idx = __builtin_bit_cast(int, mh_xor_partner<O>(__builtin_bit_cast(float, c.idx), lane));
    return r;
}
// arg-max over the 16 lanes of a DPP row (every lane gets the result)
MH_DEV Cand row16_argmax(Cand c, unsigned lane) {
    c = cand_best(c, cand_partner<8>(c, lane));
    c = cand_best(c, cand_partner<4>(c, lane));
    c = cand_best(c, cand_partner<2>(c, lane));
    c = cand_best(c, cand_partner<1>(c, lane));
    return c;
}
MH_DEV Cand wave_argmax(Cand c, unsigned lane) {
    c = cand_best(c, cand_partner<32>(c, lane));
    c = cand_best(c, cand_partner<16>(c, lane));
    return row16_argmax(c, lane);
}
MH_DEV double row16_max_f64(double v, unsigned lane) {
    v = fmax(v, mh_xor_partner_f64<8>(v, lane));
    v = fmax(v, mh_xor_partner_f64<4>(v, lane));
    v = fmax(v, mh_xor_partner_f64<2>(v, lane));
    v = fmax(v, mh_xor_partner_f64<1>(v, lane));
    return v;
}
MH_DEV double wave_max_f64(double v, unsigned lane) {
    v = fmax(v, mh_xor_partner_f64<32>(v, lane));
    v = fmax(v, mh_xor_partner_f64<16>(v, lane));
    return row16_max_f64(v, lane);
}
MH_DEV double wave_sum_f64(double v, unsigned lane) {
    v += mh_xor_partner_f64<32>(v, lane);
    v += mh_xor_partner_f64<16>(v, lane);
    v += mh_xor_partner_f64<8>(v, lane);
    v += mh_xor_partner_f64<4>(v, lane);
    v += mh_xor_partner_f64<2>(v, lane);
    v += mh_xor_partner_f64<1>(v, lane);
    return v;
}

// what a wave publishes per selection: its best candidate and that sample's state (the update needs it on every thread)
struct SvcSlot {
    double v;      // -y G (select i) or b^2 / a (select j)
    double alpha;
    double G;
    double aux;    // select i: the wave's max of y G over I_low
    float ktt;     // K[idx][idx]
    float kit;     // select j: K[i][idx]
    int ypos;
    int idx;
};

// element t = s * 1024 + tid of a Gram row through a buffer resource over its n floats.  The WHOLE byte offset is the vector
// offset: the range check of a raw buffer covers the vector and the instruction offset only, a scalar offset is added after it.  So
// a column t >= n is out of range, reads as 0, and nothing outside [row, row + 4 n) is touched.
MH_DEV float svc_row_elem(__amdgpu_buffer_rsrc_t row, int tid, int s) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(row, (s * SVC_THREADS + tid) * 4, 0, 0));
}

// AREG: alpha of the owned samples in registers (SPT <= 4).  With 8 or 16 samples per thread the registers go to G and the two rows:
// alpha then stays in the caller's buffer, read and written only by the thread that owns the sample.
template <int SPT, bool AREG>
__global__ __launch_bounds__(SVC_THREADS) void svc_smo_kernel(MhSvcProblem a) {
    __shared__ SvcSlot sel[2][SVC_WAVES];
    __shared__ double red[4][SVC_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const unsigned lane = mh_lane_id();
    double* st = a.state + (size_t)p * MH_SVC_STATE;
    if (st[0] != (double)MH_SVC_RUNNING) return;      // converged or out of iterations in an earlier launch (uniform)
    const int n = a.n;
    const size_t ldk = (size_t)a.ldk;
    const float* __restrict__ K = a.K;
    const double* __restrict__ Cv = a.Cv + (size_t)p * n;
    double* Al = a.alpha + (size_t)p * n;
    double* Gg = a.G + (size_t)p * n;

    double al[AREG ? SPT : 1], G[SPT];
    float ktt[SPT];
    unsigned ypos = 0, up = 0, low = 0, live = 0;
#pragma unroll
    for (int s = 0; s < SPT; ++s) {
        const int t = s * SVC_THREADS + tid;
        if (AREG) al[s] = 0.0;
        G[s] = 0.0; ktt[s] = 0.f;
        if (t < n) {
            const double a0 = Al[t], c = Cv[t];
            if (AREG) al[s] = a0;
            G[s] = Gg[t];
            ktt[s] = K[(size_t)t * ldk + t];
            const bool pos = a.y[t] > 0.f, below = a0 < c, above = a0 > 0.0;
            ypos |= (unsigned)pos << s;
            up |= (unsigned)(pos ? below : above) << s;
            low |= (unsigned)(pos ? above : below) << s;
            live |= (unsigned)(c > 0.0) << s;
        }
    }
    // what this thread publishes for its sample c.idx: selects over the register arrays, so nothing is indexed at run time
    auto publish = [&](Cand c, double aux, const float (&krow)[SPT], bool with_row) {
        const int slot = c.idx >> 10;
        double pa = 0.0, pg = 0.0;
        float pk = 0.f, pr = 0.f;
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            const bool m = s == slot;
            if (AREG) pa = m ? al[s] : pa;
            pg = m ? G[s] : pg;
            pk = m ? ktt[s] : pk;
            pr = m ? krow[s] : pr;
        }
        if (!AREG && c.idx != INT_MAX) pa = Al[c.idx];
        const SvcSlot w = {c.v, pa, pg, aux, pk, with_row ? pr : 0.f, (int)((ypos >> (slot & 31)) & 1u), c.idx};
        return w;
    };
    // the owner of sample t takes its new alpha and its new membership of I_up / I_low
    auto own = [&](int t, double an, double c, bool pos) {
        const int slot = t >> 10;
        const bool below = an < c, above = an > 0.0;
        if (AREG) {
#pragma unroll
            for (int s = 0; s < SPT; ++s) al[s] = s == slot ? an : al[s];
        } else {
            Al[t] = an;
        }
        up = (up & ~(1u << slot)) | ((unsigned)(pos ? below : above) << slot);
        low = (low & ~(1u << slot)) | ((unsigned)(pos ? above : below) << slot);
    };
    long long iters = (long long)st[1];
    double gap = INFINITY;
    int status = MH_SVC_RUNNING;
    for (int it = 0;; ++it) {
        // ---- i = argmax over I_up of -y G ;  Gmax2 = max over I_low of y G
        Cand ci = {-INFINITY, INT_MAX};
        double g2 = -INFINITY;
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            const double yG = ((ypos >> s) & 1u) ? G[s] : -G[s];
            if (((up >> s) & 1u) && -yG > ci.v) { ci.v = -yG; ci.idx = s * SVC_THREADS + tid; }
            if ((low >> s) & 1u) g2 = fmax(g2, yG);
        }
        ci = wave_argmax(ci, lane);
        g2 = wave_max_f64(g2, lane);
        if (lane == (unsigned)(ci.idx & 63)) sel[0][wave] = publish(ci, g2, ktt, false);
        __syncthreads();
        Cand bi = {sel[0][lane & 15].v, sel[0][lane & 15].idx};
        bi = row16_argmax(bi, lane);
        const double Gmax = bi.v, Gmax2 = row16_max_f64(sel[0][lane & 15].aux, lane);
        const int i = __builtin_amdgcn_readfirstlane(bi.idx);
        gap = (i == INT_MAX) ? 0.0 : Gmax + Gmax2;
        if (i == INT_MAX || !(gap >= a.tol)) { status = MH_SVC_CONVERGED; break; }
        if (a.max_iter >= 0 && iters >= (long long)a.max_iter) { status = MH_SVC_MAXITER; break; }
        if (it >= a.budget) break;
        const SvcSlot si = sel[0][(i & (SVC_THREADS - 1)) >> 6];
        const double Kii = (double)si.ktt, Ci = Cv[i];

        // ---- row i ;  j = argmax over {t in I_low, b_t > 0} of b_t^2 / a_t
        const __amdgpu_buffer_rsrc_t rsrc_i = mh_rsrc(K + (size_t)i * ldk, (uint32_t)n * 4u);
        float ki[SPT];
#pragma unroll
        for (int s = 0; s < SPT; ++s) ki[s] = svc_row_elem(rsrc_i, tid, s);
        // inside a thread b1^2 / q1 > b2^2 / q2 is decided as b1^2 q2 > b2^2 q1 (q > 0): one division per thread, not one per sample
        double bn = -1.0, bq = 1.0;
        int bt = INT_MAX;
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            const double yG = ((ypos >> s) & 1u) ? G[s] : -G[s];
            const double b = Gmax + yG;
            if (((low >> s) & 1u) && b > 0.0) {
                double q = Kii + (double)ktt[s] - 2.0 * (double)ki[s];
                if (!(q > 0.0)) q = SVC_TAU;
                if (b * b * bq > bn * q) { bn = b * b; bq = q; bt = s * SVC_THREADS + tid; }
            }
        }
        Cand cj = {bt == INT_MAX ? -INFINITY : bn / bq, bt};
        cj = wave_argmax(cj, lane);
        if (lane == (unsigned)(cj.idx & 63)) sel[1][wave] = publish(cj, 0.0, ki, true);
        __syncthreads();
        Cand bj = {sel[1][lane & 15].v, sel[1][lane & 15].idx};
        bj = row16_argmax(bj, lane);
        const int j = __builtin_amdgcn_readfirstlane(bj.idx);
        if (j == INT_MAX) { status = MH_SVC_CONVERGED; break; }      // cannot happen while gap >= tol > 0; never spin on it
        const SvcSlot sj = sel[1][(j & (SVC_THREADS - 1)) >> 6];
        const double Cj = Cv[j];
        const __amdgpu_buffer_rsrc_t rsrc_j = mh_rsrc(K + (size_t)j * ldk, (uint32_t)n * 4u);
        float kj[SPT];
#pragma unroll
        for (int s = 0; s < SPT; ++s) kj[s] = svc_row_elem(rsrc_j, tid, s);

        // ---- the two-variable update (libsvm Solver::Solve), on every thread alike
        double quad = Kii + (double)sj.ktt - 2.0 * (double)sj.kit;
        if (!(quad > 0.0)) quad = SVC_TAU;
        double ai = si.alpha, aj = sj.alpha;
        if (si.ypos != sj.ypos) {
            const double delta = (-si.G - sj.G) / quad, diff = ai - aj;
            ai += delta; aj += delta;
            if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
            else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
            if (diff > Ci - Cj) { if (ai > Ci) { ai = Ci; aj = Ci - diff; } }
            else { if (aj > Cj) { aj = Cj; ai = Cj + diff; } }
        } else {
            const double delta = (si.G - sj.G) / quad, sum = ai + aj;
            ai -= delta; aj += delta;
            if (sum > Ci) { if (ai > Ci) { ai = Ci; aj = sum - Ci; } }
            else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
            if (sum > Cj) { if (aj > Cj) { aj = Cj; ai = sum - Cj; } }
            else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
        }
        // Q_ti = y_t y_i K_ti
        const double di = (si.ypos ? 1.0 : -1.0) * (ai - si.alpha), dj = (sj.ypos ? 1.0 : -1.0) * (aj - sj.alpha);
#pragma unroll
        for (int s = 0; s < SPT; ++s) {
            const double d = (double)ki[s] * di + (double)kj[s] * dj;
            G[s] += ((ypos >> s) & 1u) ? d : -d;
        }
        // the owners of i and j take the new alpha and the new membership of I_up / I_low
        if ((i & (SVC_THREADS - 1)) == tid) own(i, ai, Ci, si.ypos != 0);
        if ((j & (SVC_THREADS - 1)) == tid) own(j, aj, Cj, sj.ypos != 0);
        ++iters;
    }

    // ---- leave the state behind: alpha, G, rho (libsvm calculate_rho over the samples with C > 0), the gap
    double ub = INFINITY, lb = -INFINITY, sum_free = 0.0, n_free = 0.0;
#pragma unroll
    for (int s = 0; s < SPT; ++s) {
        const int t = s * SVC_THREADS + tid;
        if (t < n) {
            if (AREG) Al[t] = al[s];
            Gg[t] = G[s];
            if ((live >> s) & 1u) {
                const double yG = ((ypos >> s) & 1u) ? G[s] : -G[s];
                const bool u = (up >> s) & 1u, l = (low >> s) & 1u;
                if (u && l) { sum_free += yG; n_free += 1.0; }
                else if (!u) lb = fmax(lb, yG);
                else ub = fmin(ub, yG);
            }
        }
    }
    ub = -wave_max_f64(-ub, lane);
    lb = wave_max_f64(lb, lane);
    sum_free = wave_sum_f64(sum_free, lane);
    n_free = wave_sum_f64(n_free, lane);
    if (lane == 0) { red[0][wave] = ub; red[1][wave] = lb; red[2][wave] = sum_free; red[3][wave] = n_free; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SVC_WAVES; ++w) {
            ub = fmin(ub, red[0][w]); lb = fmax(lb, red[1][w]); sum_free += red[2][w]; n_free += red[3][w];
        }
        st[0] = (double)status;
        st[1] = (double)iters;
        st[2] = gap;
        st[3] = n_free > 0.0 ? sum_free / n_free : (ub + lb) * 0.5;
    }
}

__global__ void svc_init_kernel(double* alpha, double* G, double* state, size_t total, int P) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) { alpha[i] = 0.0; G[i] = -1.0; }
    if (i < (size_t)P) {
        state[i * MH_SVC_STATE + 0] = (double)MH_SVC_RUNNING;
        state[i * MH_SVC_STATE + 1] = 0.0;
        state[i * MH_SVC_STATE + 2] = INFINITY;
        state[i * MH_SVC_STATE + 3] = 0.0;
    }
}

int svc_check(const MhSvcProblem* p) {
    if (!p || !p->alpha || !p->G || !p->state) return MH_EINVAL;
    if (p->n < 1 || p->n > MH_SVC_MAX_N || p->P < 1 || p->P > MH_SVC_MAX_PROBLEMS) return MH_ESHAPE;
    return MH_OK;
}

}  // namespace

extern "C" int mh_svc_init(const MhSvcProblem* p, mh_stream_t stream) {
    const int e = svc_check(p);
    if (e != MH_OK) return e;
    const size_t total = (size_t)p->P * p->n;
    hipLaunchKernelGGL(svc_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->alpha, p->G,
                       p->state, total, p->P);
    return mh_launch_status();
}

extern "C" int mh_svc_solve(const MhSvcProblem* p, mh_stream_t stream) {
    const int e = svc_check(p);
    if (e != MH_OK) return e;
    if (!p->K || !p->y || !p->Cv) return MH_EINVAL;
    if (p->ldk < p->n) return MH_ESHAPE;
    if (p->budget < 1 || !(p->tol > 0.0)) return MH_EINVAL;
    const dim3 grid(p->P), block(SVC_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const int spt = (p->n + SVC_THREADS - 1) / SVC_THREADS;
    if (spt <= 1) hipLaunchKernelGGL((svc_smo_kernel<1, true>), grid, block, 0, s, *p);
    else if (spt <= 2) hipLaunchKernelGGL((svc_smo_kernel<2, true>), grid, block, 0, s, *p);
    else if (spt <= 4) hipLaunchKernelGGL((svc_smo_kernel<4, true>), grid, block, 0, s, *p);
    else if (spt <= 8) hipLaunchKernelGGL((svc_smo_kernel<8, false>), grid, block, 0, s, *p);
    else hipLaunchKernelGGL((svc_smo_kernel<16, false>), grid, block, 0, s, *p);
    return mh_launch_status();
}
