// Discrete-output hidden Markov models: the scaled forward-backward E-step as a chunked scan, the emission sums and
// the M-step.  The contract is in include/msmhip.h and DESIGN.md ("HMM"); the tests hold it to tests/_hmm_ref.py run
// in 80-bit floats.
//
// A sequence of length T is cut into chunks of MSM_HMM_CHUNK steps (chunk c: t = 1 + cL .. min((c+1)L, T-1)).
//   products   every chunk forms P_c = prod_t A diag(b_t), rescaled by exact powers of two as it goes
//   boundaries one group of lanes per sequence walks its chunks: a_{c+1} ~ a_c P_c forwards, w_c ~ P_c w_{c+1} backwards
//   pass       every chunk replays alpha^ from a_c into LDS and walks beta^ back from w_{c+1}: gamma, one partial C,
//              one partial sum of ln c_t, gamma_0 for the first chunk of a sequence
//   folds      the partials of a sequence, then the sequences, in ascending order
// A chunk belongs to NP lanes (n padded to a power of two), lane j owning hidden state j: a wave carries 64 / NP
// chunks.  Per-lane rows and columns are indexed by unrolled loops only, so they stay in registers.  Every sum is
// taken in an order fixed by the inputs alone; no floating-point atomics.
#include <algorithm>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kL = MSM_HMM_CHUNK;
constexpr int kW = 64;               // a walk workgroup is one wave
constexpr int kFoldT = 256;
constexpr int kSeg = 256;            // member frames of an emission unit
constexpr int kRow = kSeg + 4;       // slab row stride of the emission unit (tram.hip)
constexpr int kWalkPerCu = 2;
static_assert(kL == 64 && kSeg == 256, "the staging loops and the emission row sums assume these");

template <int NP>
__device__ __forceinline__ double group_sum(double v) {   // every lane of the group ends with the same bits
#pragma unroll
    for (int off = NP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <int NP>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
    for (int off = NP / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// The two semirings of the chunk products: (+, x) for forward-backward, (max, +) on logarithms for Viterbi.
struct SumProduct {
    static constexpr bool kRescale = true;      // by exact powers of two; logarithms neither underflow nor need it
    static __device__ __forceinline__ double zero() { return 0.0; }
    static __device__ __forceinline__ double one() { return 1.0; }
    static __device__ __forceinline__ double add(double a, double b) { return a + b; }
    static __device__ __forceinline__ double mul(double a, double b) { return a * b; }
};
struct MaxPlus {
    static constexpr bool kRescale = false;
    static __device__ __forceinline__ double zero() { return -INFINITY; }
    static __device__ __forceinline__ double one() { return 0.0; }
    static __device__ __forceinline__ double add(double a, double b) { return fmax(a, b); }
    static __device__ __forceinline__ double mul(double a, double b) { return a + b; }      // -inf + x = -inf, never NaN
};

struct Tables {
    const int32_t* labels;
    int64_t N;
    int k, n;
    const int64_t* seq;          // [Q, 3] start, stride, length
    int Q;
    const int64_t* chunk_ptr;    // [Q + 1]
    const int32_t* chunk_seq;    // [n_chunks]
    int64_t n_chunks;
};

struct Seq {
    int64_t start, stride, T, c0;
    bool ok;
};

// A sequence whose triple or chunk range does not describe frames of [0, N) is not walked.
__device__ __forceinline__ Seq seq_of(const Tables& tb, int q) {
    Seq s{0, 1, 0, 0, false};
    if (q < 0 || q >= tb.Q) return s;
    s.start = tb.seq[3 * (int64_t)q];
    s.stride = tb.seq[3 * (int64_t)q + 1];
    s.T = tb.seq[3 * (int64_t)q + 2];
    s.c0 = tb.chunk_ptr[q];
    const int64_t c1 = tb.chunk_ptr[q + 1];
    s.ok = s.start >= 0 && s.start < tb.N && s.stride >= 1 && s.T >= 1 && (s.T - 1) <= (tb.N - 1 - s.start) / s.stride &&
           s.c0 >= 0 && c1 <= tb.n_chunks && c1 - s.c0 == (s.T - 1 + kL - 1) / kL;
    return s;
}

struct Chunk {
    int q, len;
    int64_t first, stride;   // frame of the chunk's first step, step between frames
    bool head;               // the sequence's first chunk
};

__device__ __forceinline__ Chunk chunk_of(const Tables& tb, int64_t ch, int& bad) {
    Chunk c{-1, 0, 0, 1, false};
    if (ch >= tb.n_chunks) return c;
    const int q = tb.chunk_seq[ch];
    const Seq s = seq_of(tb, q);
    const int64_t ci = ch - s.c0;
    if (!s.ok || ci < 0 || 1 + ci * kL > s.T - 1) {
        bad |= MSM_HMM_BAD_TABLE;
        return c;
    }
    const int64_t t0 = 1 + ci * kL, t1 = std::min<int64_t>((ci + 1) * kL, s.T - 1);
    c.q = q;
    c.len = (int)(t1 - t0 + 1);
    c.first = s.start + t0 * s.stride;
    c.stride = s.stride;
    c.head = ci == 0;
    return c;
}

// b_t(lane's state) of the chunk's steps into sb[s * 64 + lane]; the semiring's zero past the chunk and for padded states.
template <typename S>
__device__ __forceinline__ bool stage_emissions(const Tables& tb, const Chunk& cd, const double* __restrict__ B, int i,
                                                double* sb) {
    bool badsym = false;
#pragma unroll 8
    for (int s = 0; s < kL; ++s) {
        double b = S::zero();
        if (s < cd.len) {
            const int o = tb.labels[cd.first + (int64_t)s * cd.stride];
            if (o >= 0 && o < tb.k) {
                if (i < tb.n) b = B[(int64_t)i * tb.k + o];
            } else {
                badsym = true;
            }
        }
        sb[s * kW + threadIdx.x] = b;
    }
    return badsym;
}

// P_c = the semiring product over the chunk's steps of A diag(b_t); lane i of a chunk's group holds row i.
template <int NP, typename S>
__global__ __launch_bounds__(kW) void hmm_product_kernel(Tables tb, const double* __restrict__ A,
                                                         const double* __restrict__ B, double* __restrict__ P,
                                                         int32_t* __restrict__ seq_flag, int32_t* __restrict__ status) {
    __shared__ double sA[NP * NP];
    __shared__ double sb[kL * kW];
    constexpr int G = kW / NP;
    const int lane = threadIdx.x, g = lane / NP, i = lane % NP, base = g * NP;
    for (int e = lane; e < NP * NP; e += kW) {
        const int r = e / NP, c = e % NP;
        sA[e] = r < tb.n && c < tb.n ? A[r * tb.n + c] : S::zero();
    }
    int bad = 0;
    const int64_t trips = (tb.n_chunks + G - 1) / G;
    for (int64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const int64_t ch = trip * G + g;
        const Chunk cd = chunk_of(tb, ch, bad);
        __syncthreads();                      // the previous trip's reads of sb; sA on the first trip
        if (stage_emissions<S>(tb, cd, B, i, sb)) {
            bad |= MSM_HMM_BAD_SYMBOL;
            atomicOr(&seq_flag[cd.q], MSM_HMM_BAD_SYMBOL);
        }
        __syncthreads();
        const int wl = wave_max_int(cd.len);
        double Pr[NP];                        // row i of the running product
#pragma unroll
        for (int j = 0; j < NP; ++j) Pr[j] = j == i ? S::one() : S::zero();
        for (int s = 0; s < wl; ++s) {
            asm volatile("" ::: "memory");    // A is read from LDS every step: 256 hoisted entries would spill at n = 16
            double Pn[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) Pn[j] = S::zero();
#pragma unroll
            for (int m = 0; m < NP; ++m)
#pragma unroll
                for (int j = 0; j < NP; ++j) Pn[j] = S::add(Pn[j], S::mul(Pr[m], sA[m * NP + j]));
#pragma unroll
            for (int j = 0; j < NP; ++j) Pn[j] = S::mul(Pn[j], sb[s * kW + base + j]);
            int e = 0;
            if constexpr (S::kRescale) {      // exact
                double mx = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j) mx = fmax(mx, Pn[j]);
                mx = group_max<NP>(mx);
                e = mx > 0.0 && mx < INFINITY ? -ilogb(mx) : 0;
            }
            const bool act = s < cd.len;
#pragma unroll
            for (int j = 0; j < NP; ++j) Pr[j] = act ? (S::kRescale ? ldexp(Pn[j], e) : Pn[j]) : Pr[j];
        }
        if (cd.len > 0) {
            double* out = P + (ch * NP + i) * NP;
#pragma unroll
            for (int j = 0; j < NP; ++j) out[j] = Pr[j];
        }
    }
    if (bad) atomicOr(status, bad);
}

// One group of NP lanes per sequence.  Forwards: alpha^_0, then a_{c+1} = a_c P_c / sum; the entry vectors go to
// bnd_a.  Backwards: the exit vector of the last chunk is 1, w_c = P_c w_{c+1} / sum; the exit vectors go to bnd_w
// (the pass scales them so that alpha^ . beta^ = 1).  A sum that is 0 marks the sequence as having probability 0.
template <int NP>
__global__ __launch_bounds__(kW) void hmm_boundary_kernel(Tables tb, const double* __restrict__ B,
                                                          const double* __restrict__ p0, const double* __restrict__ P,
                                                          double* __restrict__ bnd_a, double* __restrict__ bnd_w,
                                                          double* __restrict__ seq_l0, double* __restrict__ seq_g0,
                                                          int32_t* __restrict__ seq_flag, double* __restrict__ gamma,
                                                          int32_t* __restrict__ status) {
    constexpr int G = kW / NP;
    const int lane = threadIdx.x, g = lane / NP, i = lane % NP, base = g * NP;
    const int q = blockIdx.x * G + g;
    const Seq sq = seq_of(tb, q);
    int bad = 0, flag = 0;
    if (q < tb.Q && !sq.ok) bad |= MSM_HMM_BAD_TABLE;
    const int nc = sq.ok ? (int)(tb.chunk_ptr[q + 1] - sq.c0) : 0;
    double a = 0.0, l0 = -INFINITY;
    if (sq.ok) {
        flag = seq_flag[q];
        const int o = tb.labels[sq.start];
        if (o >= 0 && o < tb.k) {
            if (i < tb.n) a = p0[i] * B[(int64_t)i * tb.k + o];
        } else {
            flag |= MSM_HMM_BAD_SYMBOL;
        }
    }
    {
        const double c = group_sum<NP>(a);
        if (c > 0.0 && c < INFINITY) {
            a = a / c;
            l0 = log(c);
        } else {
            a = 0.0;
            if (sq.ok && !flag) flag |= MSM_HMM_ZERO_PROB;
        }
    }
    const double a0 = a;                       // alpha^_0
    const int wl = wave_max_int(nc);
    double cur[NP], nxt[NP];
#pragma unroll
    for (int m = 0; m < NP; ++m) cur[m] = nc > 0 ? P[((sq.c0) * NP + m) * NP + i] : 0.0;
    for (int c = 0; c < wl; ++c) {
        const bool act = c < nc;
        const int64_t ch = sq.c0 + c;
        if (act) bnd_a[ch * NP + i] = a;
#pragma unroll
        for (int m = 0; m < NP; ++m) nxt[m] = c + 1 < nc ? P[((ch + 1) * NP + m) * NP + i] : 0.0;
        double u = 0.0;
#pragma unroll
        for (int m = 0; m < NP; ++m) u += __shfl(a, base + m, 64) * cur[m];
        const double s = group_sum<NP>(u);
        if (act) {
            if (s > 0.0 && s < INFINITY) {
                a = u / s;
            } else {
                a = 0.0;
                if (!flag) flag |= MSM_HMM_ZERO_PROB;
            }
        }
#pragma unroll
        for (int m = 0; m < NP; ++m) cur[m] = nxt[m];
    }
    // backwards: lane i holds row i of P_c
    double w = i < tb.n ? 1.0 : 0.0;
#pragma unroll
    for (int m = 0; m < NP; ++m) cur[m] = nc > 0 ? P[((sq.c0 + nc - 1) * NP + i) * NP + m] : 0.0;
    for (int r = 0; r < wl; ++r) {
        const int c = nc - 1 - r;              // the chunk whose exit vector w is
        const bool act = c >= 0;
        const int64_t ch = sq.c0 + c;
        if (act) bnd_w[ch * NP + i] = w;
#pragma unroll
        for (int m = 0; m < NP; ++m) nxt[m] = c - 1 >= 0 ? P[((ch - 1) * NP + i) * NP + m] : 0.0;
        double u = 0.0;
#pragma unroll
        for (int m = 0; m < NP; ++m) u += cur[m] * __shfl(w, base + m, 64);
        const double s = group_sum<NP>(u);
        if (act) w = s > 0.0 && s < INFINITY ? u / s : 0.0;
#pragma unroll
        for (int m = 0; m < NP; ++m) cur[m] = nxt[m];
    }
    if (sq.ok) {
        if (nc == 0 && i < tb.n) gamma[sq.start * tb.n + i] = flag ? 0.0 : a0;   // one frame: gamma_0 = alpha^_0
        if (nc == 0) seq_g0[(int64_t)q * NP + i] = flag ? 0.0 : a0;
        if (i == 0) {
            seq_flag[q] = flag;
            seq_l0[q] = flag ? -INFINITY : l0;
        }
    }
    bad |= flag;
    if (bad) atomicOr(status, bad);
}

// The chunk pass.  Forwards from the entry vector: u = (alpha^ A) o b_t, c_t = sum u, alpha^_t = u / c_t kept in LDS
// next to b_t.  Backwards from the exit vector, scaled so that alpha^_t1 . beta^_t1 = 1: gamma_t = alpha^_t o beta^_t,
// v = b_t o beta^_t, x_ij = A_ij v_j, Z = sum_ij alpha^_{t-1}(i) x_ij (c_t again, formed from the backward side, so
// that alpha^ . beta^ = 1 is restored at every step), C_ij += alpha^_{t-1}(i) x_ij / Z, beta^_{t-1}(i) = sum_j x_ij / Z.
// Where every symbol has one hidden state, every quotient is x / x: gamma is 0 / 1 and C counts transitions, exactly.
template <int NP>
__global__ __launch_bounds__(kW) void hmm_pass_kernel(Tables tb, const double* __restrict__ A,
                                                      const double* __restrict__ B, const double* __restrict__ bnd_a,
                                                      const double* __restrict__ bnd_w,
                                                      const int32_t* __restrict__ seq_flag, double* __restrict__ gamma,
                                                      double* __restrict__ Cpart, double* __restrict__ lpart,
                                                      double* __restrict__ seq_g0, int32_t* __restrict__ status) {
    extern __shared__ double hmm_lds[];
    double* sb = hmm_lds;                 // [kL][64]  b_t
    double* sa = sb + kL * kW;            // [kL][64]  alpha^_t
    constexpr int G = kW / NP;
    const int lane = threadIdx.x, g = lane / NP, i = lane % NP, base = g * NP;
    double Ac[NP], Ar[NP];                // column i and row i of A
#pragma unroll
    for (int m = 0; m < NP; ++m) {
        const bool in = i < tb.n && m < tb.n;
        Ac[m] = in ? A[m * tb.n + i] : 0.0;
        Ar[m] = in ? A[i * tb.n + m] : 0.0;
    }
    int bad = 0;
    const int64_t trips = (tb.n_chunks + G - 1) / G;
    for (int64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const int64_t ch = trip * G + g;
        const Chunk cd = chunk_of(tb, ch, bad);
        const bool live = cd.len > 0 && seq_flag[cd.q] == 0;
        __syncthreads();
        stage_emissions<SumProduct>(tb, cd, B, i, sb);
        __syncthreads();
        const int wl = wave_max_int(cd.len);
        const double entry = live ? bnd_a[ch * NP + i] : 0.0;
        double a = entry, lsum = 0.0;
        for (int s = 0; s < wl; ++s) {
            double u = 0.0;
#pragma unroll
            for (int m = 0; m < NP; ++m) u += __shfl(a, base + m, 64) * Ac[m];
            const double b = sb[s * kW + lane];
            u *= b;
            const double c = group_sum<NP>(u);
            if (s < cd.len) {
                const bool ok = c > 0.0 && c < INFINITY;
                a = ok ? u / c : 0.0;
                lsum += ok ? log(c) : -INFINITY;
                sa[s * kW + lane] = a;
                if (!ok && live) bad |= MSM_HMM_ZERO_PROB;
            }
        }
        double w = live ? bnd_w[ch * NP + i] : 0.0;
        {
            const double d = group_sum<NP>(a * w);
            w = d > 0.0 && d < INFINITY ? w / d : 0.0;
        }
        double Cr[NP];
#pragma unroll
        for (int m = 0; m < NP; ++m) Cr[m] = 0.0;
        for (int s = wl - 1; s >= 0; --s) {
            const bool act = s < cd.len;
            double v = 0.0, ap = 0.0;
            if (act) {
                const double gm = sa[s * kW + lane] * w;
                if (i < tb.n) gamma[(cd.first + (int64_t)s * cd.stride) * tb.n + i] = live ? gm : 0.0;
                v = sb[s * kW + lane] * w;
                ap = s > 0 ? sa[(s - 1) * kW + lane] : entry;
            }
            double X[NP], wn = 0.0;
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                X[m] = Ar[m] * __shfl(v, base + m, 64);
                wn += X[m];
            }
            // Z = sum_i alpha^_{t-1}(i) sum_j A_ij b_t(j) beta^_t(j) is c_t again; the quotients below are the
            // correctly rounded ones (q + r (T - q Z) with r = 1 / Z, Markstein), so a term that equals Z gives 1.0
            const double Z = group_sum<NP>(ap * wn);
            const bool ok = Z > 1e-280 && Z < INFINITY;
            const double r = ok ? 1.0 / Z : 0.0;
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                const double T = ap * X[m];
                double q = T * r;
                q = fma(r, fma(-q, Z, T), q);
                if (act && ok) Cr[m] += q;
            }
            if (act) w = ok ? wn / Z : 0.0;
        }
        if (cd.len > 0) {
            double* out = Cpart + (ch * NP + i) * NP;
#pragma unroll
            for (int m = 0; m < NP; ++m) out[m] = live ? Cr[m] : 0.0;
            if (i == 0) lpart[ch] = live ? lsum : -INFINITY;
            if (cd.head) {                        // gamma_0 = alpha^_0 o beta^_0
                const double g0 = live ? entry * w : 0.0;
                if (i < tb.n) gamma[(cd.first - cd.stride) * tb.n + i] = g0;
                seq_g0[(int64_t)cd.q * NP + i] = g0;
            }
        }
    }
    if (bad) atomicOr(status, bad);
}

// Sequence q: seqC = the partial C of its chunks added in ascending order, logL = ln c_0 + the partial sums likewise.
template <int NP>
__global__ __launch_bounds__(kFoldT) void hmm_fold_seq_kernel(Tables tb, const double* __restrict__ Cpart,
                                                              const double* __restrict__ lpart,
                                                              const double* __restrict__ seq_l0,
                                                              const int32_t* __restrict__ seq_flag,
                                                              double* __restrict__ seqC, double* __restrict__ logL) {
    const int q = blockIdx.x, e = threadIdx.x;
    const Seq sq = seq_of(tb, q);
    const bool live = sq.ok && seq_flag[q] == 0;
    const int64_t c0 = sq.c0, c1 = live ? tb.chunk_ptr[q + 1] : c0;
    if (e < NP * NP) {
        double acc = 0.0;
#pragma unroll 4
        for (int64_t ch = c0; ch < c1; ++ch) acc += Cpart[ch * NP * NP + e];
        seqC[(int64_t)q * NP * NP + e] = acc;
    }
    if (e == kFoldT - 1) {
        double acc = live ? seq_l0[q] : -INFINITY;
#pragma unroll 4
        for (int64_t ch = c0; ch < c1; ++ch) acc += lpart[ch];
        logL[q] = acc;
    }
}

// C, gamma0 and the total log-likelihood: the sequences added in ascending order, those that contribute nothing left out.
template <int NP>
__global__ __launch_bounds__(kFoldT) void hmm_fold_all_kernel(int n, int Q, const double* __restrict__ seqC,
                                                              const double* __restrict__ seq_g0,
                                                              const double* __restrict__ logL,
                                                              const int32_t* __restrict__ seq_flag,
                                                              double* __restrict__ C, double* __restrict__ gamma0,
                                                              double* __restrict__ total) {
    const int e = threadIdx.x;
    if (e < NP * NP) {
        const int r = e / NP, c = e % NP;
        double acc = 0.0;
        for (int q = 0; q < Q; ++q)
            if (seq_flag[q] == 0) acc += seqC[(int64_t)q * NP * NP + e];
        if (r < n && c < n) C[r * n + c] = acc;
    }
    if (e >= kFoldT - NP - 1 && e < kFoldT - 1) {   // NP threads from the far end of the workgroup
        const int j = e - (kFoldT - NP - 1);
        double acc = 0.0;
        for (int q = 0; q < Q; ++q)
            if (seq_flag[q] == 0) acc += seq_g0[(int64_t)q * NP + j];
        if (j < n) gamma0[j] = acc;
    }
    if (e == kFoldT - 1 && total) {
        double acc = 0.0;
        for (int q = 0; q < Q; ++q) acc += logL[q];
        total[0] = acc;
    }
}

// Emission sums, the unit (symbol, segment of 256 member frames) as in tram_pass: part[unit, i] = the unit's rows of
// gamma added in the fixed order of the slab's row sums.
__global__ __launch_bounds__(kSeg) void hmm_emission_kernel(const double* __restrict__ gamma, int64_t N, int n, int k,
                                                            const int64_t* __restrict__ off,
                                                            const int32_t* __restrict__ members,
                                                            const int64_t* __restrict__ unit_ptr,
                                                            const int32_t* __restrict__ unit_state, int64_t units,
                                                            double* __restrict__ part) {
    extern __shared__ double hmm_lds[];
    double* slab = hmm_lds;                    // [n][kRow]
    double* rows = slab + (size_t)n * kRow;    // [4 waves][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* colp = slab + tid;
    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const int y = unit_state[unit];
        int64_t n0 = 0, n1 = 0;
        if (y >= 0 && y < k) {
            const int64_t o0 = off[y], o1 = off[y + 1], q = unit - unit_ptr[y];
            if (o0 >= 0 && o1 <= N && q >= 0 && q <= (o1 - o0) / kSeg) {
                n0 = o0 + q * kSeg;
                n1 = n0 + kSeg < o1 ? n0 + kSeg : o1;
            }
        }
        __syncthreads();
        int64_t f = n0 + tid < n1 ? members[n0 + tid] : -1;
        if (f >= N) f = -1;
        for (int i = 0; i < n; ++i) colp[i * kRow] = f >= 0 ? gamma[f * n + i] : 0.0;
        __syncthreads();
        if (lane < n) {
            const double* row = slab + (size_t)lane * kRow + wave * 64;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
            for (int c = 0; c < 64; c += 4) {
                a0 += row[(c + lane) & 63];
                a1 += row[(c + 1 + lane) & 63];
                a2 += row[(c + 2 + lane) & 63];
                a3 += row[(c + 3 + lane) & 63];
            }
            rows[wave * 64 + lane] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        if (tid < n) part[unit * n + tid] = ((rows[tid] + rows[64 + tid]) + rows[128 + tid]) + rows[192 + tid];
    }
}

// E[i, y] = the partial sums of symbol y's units, added in ascending unit order.
__global__ __launch_bounds__(kFoldT) void hmm_emission_fold_kernel(const double* __restrict__ part, int n, int k,
                                                                   const int64_t* __restrict__ unit_ptr, int64_t units,
                                                                   double* __restrict__ E) {
    const int64_t id = (int64_t)blockIdx.x * kFoldT + threadIdx.x;
    if (id >= (int64_t)n * k) return;
    const int i = (int)(id / k), y = (int)(id % k);
    const int64_t p0 = unit_ptr[y], p1 = unit_ptr[y + 1];
    const int64_t u0 = p0 > 0 ? p0 : 0, u1 = p1 < units ? p1 : units;
    double a = 0.0;
    for (int64_t w = u0; w < u1; ++w) a += part[w * n + i];
    E[id] = a;
}

// The M-step by one workgroup.  B: rows of E over their sums (thread-strided partial sums, block_sum_bcast).  A: the
// rows of C over their sums, or the reversible fixed point of msm_reversible_mle on C (thread a owns row a; checked
// every iteration as the batched kernel does).  pi: the fixed point's x, or the GTH elimination of the new A by
// thread 0 (no subtractions).  p0: gamma0 / Q, or pi.
__global__ __launch_bounds__(kFoldT) void hmm_mstep_kernel(int n, int k, int Q, const double* __restrict__ C,
                                                           const double* __restrict__ E,
                                                           const double* __restrict__ gamma0, int reversible,
                                                           int stationary, int maxiter, double maxerr,
                                                           double* __restrict__ A, double* __restrict__ B,
                                                           double* __restrict__ p0, double* __restrict__ pi,
                                                           int32_t* __restrict__ status) {
    constexpr int M = MSM_HMM_MAX_HIDDEN;
    __shared__ double red[kFoldT / 64];
    __shared__ double bc;
    __shared__ double sA[M * M], sG[M * M], sC2[M * M], sc[M], sv[M], sxn[M], sx[M], spi[M];
    __shared__ int sflag;
    const int tid = threadIdx.x;
    int bad = 0;
    if (tid == 0) sflag = 0;
    for (int i = 0; i < n; ++i) {
        double part = 0.0;
        for (int y = tid; y < k; y += kFoldT) part += E[(int64_t)i * k + y];
        const double rs = block_sum_bcast(part, red, &bc);
        if (rs > 0.0 && rs < INFINITY) {
            for (int y = tid; y < k; y += kFoldT) B[(int64_t)i * k + y] = E[(int64_t)i * k + y] / rs;
        } else {
            bad |= MSM_HMM_EMPTY_STATE;
        }
        __syncthreads();
    }
    for (int e = tid; e < n * n; e += kFoldT) sA[e] = A[e];
    __syncthreads();
    if (!reversible) {
        if (tid < n) {
            double rs = 0.0;
            for (int j = 0; j < n; ++j) rs += C[tid * n + j];
            if (rs > 0.0 && rs < INFINITY) {
                for (int j = 0; j < n; ++j) sA[tid * n + j] = C[tid * n + j] / rs;
            } else {
                bad |= MSM_HMM_EMPTY_STATE;
            }
        }
        __syncthreads();
        if (tid == 0) {                       // GTH: the stationary vector of sA
            for (int e = 0; e < n * n; ++e) sG[e] = sA[e];
            bool ok = true;
            for (int m = n - 1; m >= 1 && ok; --m) {
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += sG[m * n + j];
                if (!(s > 0.0)) { ok = false; break; }
                for (int r = 0; r < m; ++r) sG[r * n + m] /= s;
                for (int r = 0; r < m; ++r)
                    for (int j = 0; j < m; ++j) sG[r * n + j] += sG[r * n + m] * sG[m * n + j];
            }
            if (ok) {
                spi[0] = 1.0;
                double tot = 1.0;
                for (int m = 1; m < n; ++m) {
                    double s = 0.0;
                    for (int r = 0; r < m; ++r) s += spi[r] * sG[r * n + m];
                    spi[m] = s;
                    tot += s;
                }
                for (int m = 0; m < n; ++m) spi[m] /= tot;
            } else {
                for (int m = 0; m < n; ++m) spi[m] = 1.0 / n;      // A does not have one stationary vector
                sflag = MSM_HMM_NOT_CONVERGED;
            }
        }
        __syncthreads();
    } else {
        for (int e = tid; e < n * n; e += kFoldT) sC2[e] = C[e] + C[(e % n) * n + e / n];
        if (tid < n) {
            double cs = 0.0;
            for (int j = 0; j < n; ++j) cs += C[tid * n + j];
            sc[tid] = cs;
        }
        __syncthreads();
        if (tid < n) {
            double xs = 0.0;
            for (int j = 0; j < n; ++j) xs += sC2[tid * n + j];
            sxn[tid] = xs;
        }
        __syncthreads();
        int it = 0;
        while (true) {
            double tot = 0.0;
            for (int j = 0; j < n; ++j) tot += sxn[j];
            double worst = 0.0, x = 0.0;
            if (tid < n) {
                x = sxn[tid] / tot;
                if (it > 0) {
                    const double old = sx[tid], mid = 0.5 * (old + x);
                    if (mid > 0.0) worst = fabs(old - x) / mid;
                }
                if (!(x == x)) worst = INFINITY;
            }
            const double err = block_reduce_bcast(worst, red, &bc, 0.0, op_max{});   // barriers: sxn, sx were read
            if (tid < n) {
                sx[tid] = x;
                sv[tid] = x > 0.0 ? sc[tid] / x : 0.0;
            }
            __syncthreads();
            if (it > 0 && (!(err > maxerr) || !(err <= 4.0))) break;
            if (it >= maxiter) {
                if (tid == 0) sflag = MSM_HMM_NOT_CONVERGED;
                break;
            }
            if (tid < n) {
                double acc = 0.0;
                for (int j = 0; j < n; ++j) {
                    const double c2 = sC2[tid * n + j], den = sv[tid] + sv[j];
                    if (c2 > 0.0 && den > 0.0) acc += c2 / den;
                }
                sxn[tid] = acc;
            }
            ++it;
            __syncthreads();
        }
        if (tid < n) {
            double acc = 0.0;
            for (int j = 0; j < n; ++j) {
                const double c2 = sC2[tid * n + j], den = sv[tid] + sv[j];
                if (c2 > 0.0 && den > 0.0) acc += c2 / den;
            }
            if (acc > 0.0 && acc < INFINITY) {
                for (int j = 0; j < n; ++j) {
                    const double c2 = sC2[tid * n + j], den = sv[tid] + sv[j];
                    sA[tid * n + j] = (c2 > 0.0 && den > 0.0) ? (c2 / den) / acc : 0.0;
                }
            } else {
                bad |= MSM_HMM_EMPTY_STATE;
            }
            spi[tid] = sx[tid];
        }
        __syncthreads();
    }
    for (int e = tid; e < n * n; e += kFoldT) A[e] = sA[e];
    if (tid < n) {
        pi[tid] = spi[tid];
        p0[tid] = stationary ? spi[tid] : gamma0[tid] / (double)Q;
    }
    __syncthreads();
    bad |= sflag;
    if (bad) atomicOr(status, bad);
}

// ---- Viterbi: the same chunking in the (max, +) semiring on ln A, ln B, ln p0 ----------------------------------------
__global__ __launch_bounds__(kFoldT) void hmm_log_kernel(int64_t n, const double* __restrict__ src,
                                                         double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kFoldT + threadIdx.x;
    if (i < n) dst[i] = src[i] > 0.0 ? log(src[i]) : -INFINITY;
}

// the largest of the group's values and the lowest lane that holds it, in every lane of the group
template <int NP>
__device__ __forceinline__ void group_argmax(double v, int base, double& best, int& at) {
    best = -INFINITY;
    at = 0;
#pragma unroll
    for (int m = 0; m < NP; ++m) {
        const double x = __shfl(v, base + m, 64);
        if (x > best) { best = x; at = m; }
    }
}

// One group per sequence.  Forwards: delta_0 = ln p0 + ln b_0, delta_{c+1}(j) = max_i delta_c(i) + P_c(i, j); the
// entry vectors stay in bnd_d.  Backwards: the last state is argmax delta, then s_c = argmax_i delta_c(i) + P_c(i,
// s_{c+1}); bnd_s[ch] = {state on entry (at the step before the chunk), state at the chunk's last step}.
template <int NP>
__global__ __launch_bounds__(kW) void hmm_viterbi_boundary_kernel(Tables tb, const double* __restrict__ lB,
                                                                  const double* __restrict__ lp0,
                                                                  const double* __restrict__ P,
                                                                  double* __restrict__ bnd_d,
                                                                  int32_t* __restrict__ bnd_s,
                                                                  int32_t* __restrict__ seq_flag,
                                                                  int32_t* __restrict__ path,
                                                                  double* __restrict__ logp,
                                                                  int32_t* __restrict__ status) {
    constexpr int G = kW / NP;
    const int lane = threadIdx.x, g = lane / NP, i = lane % NP, base = g * NP;
    const int q = blockIdx.x * G + g;
    const Seq sq = seq_of(tb, q);
    int bad = 0, flag = 0;
    if (q < tb.Q && !sq.ok) bad |= MSM_HMM_BAD_TABLE;
    const int nc = sq.ok ? (int)(tb.chunk_ptr[q + 1] - sq.c0) : 0;
    double d = -INFINITY;
    if (sq.ok) {
        flag = seq_flag[q];
        const int o = tb.labels[sq.start];
        if (o >= 0 && o < tb.k) {
            if (i < tb.n) d = lp0[i] + lB[(int64_t)i * tb.k + o];
        } else {
            flag |= MSM_HMM_BAD_SYMBOL;
        }
    }
    const int wl = wave_max_int(nc);
    double cur[NP], nxt[NP];
#pragma unroll
    for (int m = 0; m < NP; ++m) cur[m] = nc > 0 ? P[((sq.c0) * NP + m) * NP + i] : -INFINITY;
    for (int c = 0; c < wl; ++c) {
        const bool act = c < nc;
        const int64_t ch = sq.c0 + c;
        if (act) bnd_d[ch * NP + i] = d;
#pragma unroll
        for (int m = 0; m < NP; ++m) nxt[m] = c + 1 < nc ? P[((ch + 1) * NP + m) * NP + i] : -INFINITY;
        double u = -INFINITY;
#pragma unroll
        for (int m = 0; m < NP; ++m) u = fmax(u, __shfl(d, base + m, 64) + cur[m]);
        if (act) d = u;
#pragma unroll
        for (int m = 0; m < NP; ++m) cur[m] = nxt[m];
    }
    double best;
    int state;
    group_argmax<NP>(d, base, best, state);
    if (sq.ok && !flag && !(best > -INFINITY)) flag |= MSM_HMM_ZERO_PROB;
    const int last = state;
    // backwards: lane i holds row i of P_c and its own delta_c(i)
#pragma unroll
    for (int m = 0; m < NP; ++m) cur[m] = nc > 0 ? P[((sq.c0 + nc - 1) * NP + i) * NP + m] : -INFINITY;
    for (int r = 0; r < wl; ++r) {
        const int c = nc - 1 - r;
        const bool act = c >= 0;
        const int64_t ch = sq.c0 + c;
#pragma unroll
        for (int m = 0; m < NP; ++m) nxt[m] = c - 1 >= 0 ? P[((ch - 1) * NP + i) * NP + m] : -INFINITY;
        double pick = -INFINITY;
#pragma unroll
        for (int m = 0; m < NP; ++m) pick = m == state ? cur[m] : pick;
        const double v = act ? bnd_d[ch * NP + i] + pick : -INFINITY;
        double b2;
        int from;
        group_argmax<NP>(v, base, b2, from);
        if (act) {
            if (i == 0) {
                bnd_s[2 * ch] = from;
                bnd_s[2 * ch + 1] = state;
            }
            state = from;
        }
#pragma unroll
        for (int m = 0; m < NP; ++m) cur[m] = nxt[m];
    }
    if (sq.ok && i == 0) {
        if (nc == 0) path[sq.start] = flag ? -1 : last;
        seq_flag[q] = flag;
        if (logp) logp[q] = flag ? -INFINITY : best;
    }
    bad |= flag;
    if (bad) atomicOr(status, bad);
}

// Every chunk replays delta from the one-hot entry state with back-pointers in LDS, then lane 0 of its group
// backtracks from the state at the chunk's last step.  Ties go to the lowest index.
template <int NP>
__global__ __launch_bounds__(kW) void hmm_viterbi_pass_kernel(Tables tb, const double* __restrict__ lA,
                                                              const double* __restrict__ lB,
                                                              const int32_t* __restrict__ bnd_s,
                                                              const int32_t* __restrict__ seq_flag,
                                                              int32_t* __restrict__ path, int32_t* __restrict__ status) {
    __shared__ double sb[kL * kW];
    __shared__ unsigned char bp[kL * kW];
    constexpr int G = kW / NP;
    const int lane = threadIdx.x, g = lane / NP, i = lane % NP, base = g * NP;
    double Ac[NP];
#pragma unroll
    for (int m = 0; m < NP; ++m) Ac[m] = i < tb.n && m < tb.n ? lA[m * tb.n + i] : -INFINITY;
    int bad = 0;
    const int64_t trips = (tb.n_chunks + G - 1) / G;
    for (int64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const int64_t ch = trip * G + g;
        const Chunk cd = chunk_of(tb, ch, bad);
        const bool live = cd.len > 0 && seq_flag[cd.q] == 0;
        __syncthreads();
        stage_emissions<MaxPlus>(tb, cd, lB, i, sb);
        __syncthreads();
        const int wl = wave_max_int(cd.len);
        const int enter = live ? bnd_s[2 * ch] & (NP - 1) : 0, leave = live ? bnd_s[2 * ch + 1] & (NP - 1) : 0;
        double d = live && i == enter ? 0.0 : -INFINITY;
        for (int s = 0; s < wl; ++s) {
            double best = -INFINITY;
            int from = 0;
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                const double x = __shfl(d, base + m, 64) + Ac[m];
                if (x > best) { best = x; from = m; }
            }
            if (s < cd.len) {
                d = best + sb[s * kW + lane];
                bp[s * kW + lane] = (unsigned char)from;
            }
        }
        __syncthreads();
        if (i == 0 && cd.len > 0) {
            int state = leave;
            for (int s = cd.len - 1; s >= 0; --s) {
                path[cd.first + (int64_t)s * cd.stride] = live ? state : -1;
                state = bp[s * kW + base + state] & (NP - 1);
            }
            if (cd.head) path[cd.first - cd.stride] = live ? state : -1;
        }
    }
    if (bad) atomicOr(status, bad);
}

struct ViterbiWork {
    double *lA, *lB, *lp0, *P, *bnd_d;
    int32_t *bnd_s, *seq_flag;
    size_t bytes;
};

int padded(int n);

ViterbiWork carve_viterbi(void* base, int n, int k, int64_t n_chunks, int Q) {
    const int64_t NP = padded(n), c = std::max<int64_t>(n_chunks, 1), q = std::max(Q, 1);
    ViterbiWork w;
    double* p = (double*)base;
    w.lA = p; p += (int64_t)n * n;
    w.lB = p; p += (int64_t)n * k;
    w.lp0 = p; p += n;
    w.P = p; p += c * NP * NP;
    w.bnd_d = p; p += c * NP;
    w.bnd_s = (int32_t*)p; p += c;
    w.seq_flag = (int32_t*)p; p += (q + 1) / 2;
    w.bytes = (size_t)((char*)p - (char*)base);
    return w;
}

int padded(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16; }

struct Work {
    double *P, *bnd_a, *bnd_w, *Cpart, *lpart, *seqC, *seq_g0, *seq_l0, *logL, *Epart;
    int32_t* seq_flag;
    size_t bytes;
};

Work carve(void* base, int n, int64_t n_chunks, int Q, int64_t units) {
    const int64_t NP = padded(n), c = std::max<int64_t>(n_chunks, 1), q = std::max(Q, 1);
    Work w;
    double* p = (double*)base;
    w.P = p; p += c * NP * NP;
    w.bnd_a = p; p += c * NP;
    w.bnd_w = p; p += c * NP;
    w.Cpart = p; p += c * NP * NP;
    w.lpart = p; p += c;
    w.seqC = p; p += q * NP * NP;
    w.seq_g0 = p; p += q * NP;
    w.seq_l0 = p; p += q;
    w.logL = p; p += q;
    w.Epart = p; p += std::max<int64_t>(units, 1) * n;
    w.seq_flag = (int32_t*)p; p += (q + 1) / 2;
    w.bytes = (size_t)((char*)p - (char*)base);
    return w;
}

constexpr size_t kPassLds = (size_t)2 * kL * kW * sizeof(double);

int walk_grid(const msm_ctx* ctx, int n, int64_t n_chunks, int max_workgroups) {
    const int G = kW / padded(n);
    const int64_t trips = (n_chunks + G - 1) / G;
    const int64_t cap = max_workgroups > 0 ? max_workgroups : (int64_t)ctx->n_cu * kWalkPerCu;
    return (int)std::max<int64_t>(1, std::min(trips, cap));
}

msm_status check_model(msm_ctx* ctx, const char* who, int n, int k) {
    MSM_REQUIRE(ctx, n >= 1 && k >= 1, "%s: need n >= 1 and k >= 1 (n=%d k=%d)", who, n, k);
    if (n > MSM_HMM_MAX_HIDDEN)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %d hidden states, at most %d are supported", who, n,
                        MSM_HMM_MAX_HIDDEN);
    return MSM_OK;
}

template <int NP>
msm_status estep_launch(msm_ctx* ctx, const Tables& tb, const double* A, const double* B, const double* p0,
                        int max_workgroups, const Work& w, double* gamma, double* C, double* gamma0, double* logL,
                        double* total, int32_t* status) {
    constexpr int G = kW / NP;
    MSM_HIP(ctx, hipMemsetAsync(w.seq_flag, 0, (size_t)tb.Q * sizeof(int32_t), ctx->stream));
    const int grid = walk_grid(ctx, tb.n, tb.n_chunks, max_workgroups);
    if (tb.n_chunks > 0)
        hipLaunchKernelGGL((hmm_product_kernel<NP, SumProduct>), dim3(grid), dim3(kW), 0, ctx->stream, tb, A, B, w.P, w.seq_flag,
                           status);
    hipLaunchKernelGGL(hmm_boundary_kernel<NP>, dim3(msm_ceil_div(tb.Q, G)), dim3(kW), 0, ctx->stream, tb, B, p0,
                       (const double*)w.P, w.bnd_a, w.bnd_w, w.seq_l0, w.seq_g0, w.seq_flag, gamma, status);
    MSM_CHECK_LAUNCH(ctx);
    if (tb.n_chunks > 0) {
        MSM_HIP(ctx, hipFuncSetAttribute((const void*)hmm_pass_kernel<NP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kPassLds));
        hipLaunchKernelGGL(hmm_pass_kernel<NP>, dim3(grid), dim3(kW), kPassLds, ctx->stream, tb, A, B,
                           (const double*)w.bnd_a, (const double*)w.bnd_w, (const int32_t*)w.seq_flag, gamma, w.Cpart,
                           w.lpart, w.seq_g0, status);
    }
    hipLaunchKernelGGL(hmm_fold_seq_kernel<NP>, dim3(tb.Q), dim3(kFoldT), 0, ctx->stream, tb, (const double*)w.Cpart,
                       (const double*)w.lpart, (const double*)w.seq_l0, (const int32_t*)w.seq_flag, w.seqC, logL);
    hipLaunchKernelGGL(hmm_fold_all_kernel<NP>, dim3(1), dim3(kFoldT), 0, ctx->stream, tb.n, tb.Q,
                       (const double*)w.seqC, (const double*)w.seq_g0, (const double*)logL,
                       (const int32_t*)w.seq_flag, C, gamma0, total);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status estep_dispatch(msm_ctx* ctx, const Tables& tb, const double* A, const double* B, const double* p0,
                          int max_workgroups, const Work& w, double* gamma, double* C, double* gamma0, double* logL,
                          double* total, int32_t* status) {
    switch (padded(tb.n)) {
        case 1: return estep_launch<1>(ctx, tb, A, B, p0, max_workgroups, w, gamma, C, gamma0, logL, total, status);
        case 2: return estep_launch<2>(ctx, tb, A, B, p0, max_workgroups, w, gamma, C, gamma0, logL, total, status);
        case 4: return estep_launch<4>(ctx, tb, A, B, p0, max_workgroups, w, gamma, C, gamma0, logL, total, status);
        case 8: return estep_launch<8>(ctx, tb, A, B, p0, max_workgroups, w, gamma, C, gamma0, logL, total, status);
        default: return estep_launch<16>(ctx, tb, A, B, p0, max_workgroups, w, gamma, C, gamma0, logL, total, status);
    }
}

msm_status check_tables(msm_ctx* ctx, const char* who, int64_t N, int Q, int64_t n_chunks, int max_workgroups) {
    MSM_REQUIRE(ctx, N >= 1 && Q >= 1 && Q <= N, "%s: need N >= 1 and 1 <= Q <= N (N=%lld Q=%d)", who, (long long)N, Q);
    MSM_REQUIRE(ctx, n_chunks >= 0 && n_chunks <= N, "%s: need 0 <= n_chunks <= N (n_chunks=%lld)", who,
                (long long)n_chunks);
    MSM_REQUIRE(ctx, max_workgroups >= 0, "%s: max_workgroups must be >= 0 (0: the default)", who);
    return MSM_OK;
}

msm_status emissions_launch(msm_ctx* ctx, const double* gamma, int64_t N, int n, int k, const int64_t* off,
                            const int32_t* members, const int64_t* unit_ptr, const int32_t* unit_state, int64_t units,
                            int max_workgroups, double* part, double* E) {
    const size_t lds = ((size_t)n * kRow + kSeg) * sizeof(double);
    const int64_t cap = max_workgroups > 0 ? max_workgroups : (int64_t)ctx->n_cu * 4;
    if (units > 0)
        hipLaunchKernelGGL(hmm_emission_kernel, dim3((int)std::max<int64_t>(1, std::min(units, cap))), dim3(kSeg), lds,
                           ctx->stream, gamma, N, n, k, off, members, unit_ptr, unit_state, units, part);
    hipLaunchKernelGGL(hmm_emission_fold_kernel, dim3(msm_ceil_div((int64_t)n * k, kFoldT)), dim3(kFoldT), 0,
                       ctx->stream, (const double*)part, n, k, unit_ptr, units, E);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

template <int NP>
msm_status viterbi_launch(msm_ctx* ctx, const Tables& tb, const double* A, const double* B, const double* p0,
                          int max_workgroups, const ViterbiWork& w, int32_t* path, double* logp, int32_t* status) {
    constexpr int G = kW / NP;
    MSM_HIP(ctx, hipMemsetAsync(w.seq_flag, 0, (size_t)tb.Q * sizeof(int32_t), ctx->stream));
    MSM_HIP(ctx, hipMemsetAsync(path, 0xFF, (size_t)tb.N * sizeof(int32_t), ctx->stream));
    const int64_t nn = (int64_t)tb.n * tb.n, nk = (int64_t)tb.n * tb.k;
    hipLaunchKernelGGL(hmm_log_kernel, dim3(msm_ceil_div(nn, kFoldT)), dim3(kFoldT), 0, ctx->stream, nn, A, w.lA);
    hipLaunchKernelGGL(hmm_log_kernel, dim3(msm_ceil_div(nk, kFoldT)), dim3(kFoldT), 0, ctx->stream, nk, B, w.lB);
    hipLaunchKernelGGL(hmm_log_kernel, dim3(1), dim3(kFoldT), 0, ctx->stream, (int64_t)tb.n, p0, w.lp0);
    const int grid = walk_grid(ctx, tb.n, tb.n_chunks, max_workgroups);
    if (tb.n_chunks > 0)
        hipLaunchKernelGGL((hmm_product_kernel<NP, MaxPlus>), dim3(grid), dim3(kW), 0, ctx->stream, tb,
                           (const double*)w.lA, (const double*)w.lB, w.P, w.seq_flag, status);
    hipLaunchKernelGGL(hmm_viterbi_boundary_kernel<NP>, dim3(msm_ceil_div(tb.Q, G)), dim3(kW), 0, ctx->stream, tb,
                       (const double*)w.lB, (const double*)w.lp0, (const double*)w.P, w.bnd_d, w.bnd_s, w.seq_flag,
                       path, logp, status);
    if (tb.n_chunks > 0)
        hipLaunchKernelGGL(hmm_viterbi_pass_kernel<NP>, dim3(grid), dim3(kW), 0, ctx->stream, tb, (const double*)w.lA,
                           (const double*)w.lB, (const int32_t*)w.bnd_s, (const int32_t*)w.seq_flag, path, status);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // namespace

extern "C" {

size_t msm_hmm_viterbi_workspace_bytes(int n, int k, int64_t n_chunks, int Q) {
    if (n < 1 || n > MSM_HMM_MAX_HIDDEN || k < 1 || n_chunks < 0 || Q < 0) return 0;
    return carve_viterbi(nullptr, n, k, n_chunks, Q).bytes;
}

msm_status msm_hmm_viterbi(msm_ctx* ctx, const int32_t* d_labels, int64_t N, int k, int n, const int64_t* d_seq, int Q,
                           const int64_t* d_chunk_ptr, const int32_t* d_chunk_seq, int64_t n_chunks, const double* d_A,
                           const double* d_B, const double* d_p0, int max_workgroups, void* d_work, int32_t* d_path,
                           double* d_logp, int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_model(ctx, "msm_hmm_viterbi", n, k);
    if (rs != MSM_OK) return rs;
    rs = check_tables(ctx, "msm_hmm_viterbi", N, Q, n_chunks, max_workgroups);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, d_labels && d_seq && d_chunk_ptr && (d_chunk_seq || n_chunks == 0) && d_A && d_B && d_p0 && d_work &&
                         d_path && d_status, "msm_hmm_viterbi: NULL pointer");
    const Tables tb{d_labels, N, k, n, d_seq, Q, d_chunk_ptr, d_chunk_seq, n_chunks};
    const ViterbiWork w = carve_viterbi(d_work, n, k, n_chunks, Q);
    switch (padded(n)) {
        case 1: return viterbi_launch<1>(ctx, tb, d_A, d_B, d_p0, max_workgroups, w, d_path, d_logp, d_status);
        case 2: return viterbi_launch<2>(ctx, tb, d_A, d_B, d_p0, max_workgroups, w, d_path, d_logp, d_status);
        case 4: return viterbi_launch<4>(ctx, tb, d_A, d_B, d_p0, max_workgroups, w, d_path, d_logp, d_status);
        case 8: return viterbi_launch<8>(ctx, tb, d_A, d_B, d_p0, max_workgroups, w, d_path, d_logp, d_status);
        default: return viterbi_launch<16>(ctx, tb, d_A, d_B, d_p0, max_workgroups, w, d_path, d_logp, d_status);
    }
}

size_t msm_hmm_workspace_bytes(int n, int64_t n_chunks, int Q, int64_t units) {
    if (n < 1 || n > MSM_HMM_MAX_HIDDEN || n_chunks < 0 || Q < 0 || units < 0) return 0;
    return carve(nullptr, n, n_chunks, Q, units).bytes;
}

msm_status msm_hmm_plan(msm_ctx* ctx, int n, int64_t n_chunks, int Q, int max_workgroups, int64_t out[8]) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, out, "msm_hmm_plan: NULL pointer");
    const msm_status rs = check_model(ctx, "msm_hmm_plan", n, 1);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, n_chunks >= 0 && Q >= 1 && max_workgroups >= 0, "msm_hmm_plan: need n_chunks >= 0, Q >= 1 and max_workgroups >= 0");
    const int NP = padded(n);
    out[0] = kL;
    out[1] = NP;
    out[2] = n_chunks;
    out[3] = walk_grid(ctx, n, n_chunks, max_workgroups);                       // products and pass
    out[4] = msm_ceil_div(Q, kW / NP);                                          // boundaries
    out[5] = (int64_t)(kL * kW + NP * NP) * (int64_t)sizeof(double);            // LDS bytes of the products
    out[6] = (int64_t)kPassLds;                                                 // LDS bytes of the pass
    out[7] = ((int64_t)n * kRow + kSeg) * (int64_t)sizeof(double);              // LDS bytes of an emission unit
    return MSM_OK;
}

msm_status msm_hmm_estep(msm_ctx* ctx, const int32_t* d_labels, int64_t N, int k, int n, const int64_t* d_seq, int Q,
                         const int64_t* d_chunk_ptr, const int32_t* d_chunk_seq, int64_t n_chunks, const double* d_A,
                         const double* d_B, const double* d_p0, int max_workgroups, void* d_work, double* d_gamma,
                         double* d_C, double* d_gamma0, double* d_logL, double* d_total, int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_model(ctx, "msm_hmm_estep", n, k);
    if (rs != MSM_OK) return rs;
    rs = check_tables(ctx, "msm_hmm_estep", N, Q, n_chunks, max_workgroups);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, d_labels && d_seq && d_chunk_ptr && (d_chunk_seq || n_chunks == 0) && d_A && d_B && d_p0 && d_work &&
                         d_gamma && d_C && d_gamma0 && d_logL && d_status, "msm_hmm_estep: NULL pointer");
    const Tables tb{d_labels, N, k, n, d_seq, Q, d_chunk_ptr, d_chunk_seq, n_chunks};
    return estep_dispatch(ctx, tb, d_A, d_B, d_p0, max_workgroups, carve(d_work, n, n_chunks, Q, 0), d_gamma, d_C,
                          d_gamma0, d_logL, d_total, d_status);
}

msm_status msm_hmm_emissions(msm_ctx* ctx, const double* d_gamma, int64_t N, int n, int k, const int64_t* d_offsets,
                             const int32_t* d_members, const int64_t* d_unit_ptr, const int32_t* d_unit_state,
                             int64_t units, int max_workgroups, double* d_part, double* d_E) {
    if (!ctx) return MSM_ERR_INVALID;
    const msm_status rs = check_model(ctx, "msm_hmm_emissions", n, k);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, N >= 1 && units >= 0 && units <= N + k && max_workgroups >= 0,
                "msm_hmm_emissions: need N >= 1, 0 <= units <= N + k and max_workgroups >= 0");
    MSM_REQUIRE(ctx, d_gamma && d_offsets && d_members && d_unit_ptr && (d_unit_state || units == 0) && d_part && d_E,
                "msm_hmm_emissions: NULL pointer");
    return emissions_launch(ctx, d_gamma, N, n, k, d_offsets, d_members, d_unit_ptr, d_unit_state, units,
                            max_workgroups, d_part, d_E);
}

msm_status msm_hmm_mstep(msm_ctx* ctx, int n, int k, int Q, const double* d_C, const double* d_E,
                         const double* d_gamma0, int reversible, int stationary, int maxiter, double maxerr,
                         double* d_A, double* d_B, double* d_p0, double* d_pi, int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    const msm_status rs = check_model(ctx, "msm_hmm_mstep", n, k);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, Q >= 1 && maxiter >= 1 && maxiter <= MSM_HMM_MAX_FIXED_POINT && maxerr >= 0.0,
                "msm_hmm_mstep: need Q >= 1, 1 <= maxiter <= %d and maxerr >= 0", MSM_HMM_MAX_FIXED_POINT);
    MSM_REQUIRE(ctx, d_C && d_E && d_gamma0 && d_A && d_B && d_p0 && d_pi && d_status, "msm_hmm_mstep: NULL pointer");
    hipLaunchKernelGGL(hmm_mstep_kernel, dim3(1), dim3(kFoldT), 0, ctx->stream, n, k, Q, d_C, d_E, d_gamma0, reversible,
                       stationary, maxiter, maxerr, d_A, d_B, d_p0, d_pi, d_status);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_hmm_iterations(msm_ctx* ctx, const int32_t* d_labels, int64_t N, int k, int n, const int64_t* d_seq,
                              int Q, const int64_t* d_chunk_ptr, const int32_t* d_chunk_seq, int64_t n_chunks,
                              const int64_t* d_offsets, const int32_t* d_members, const int64_t* d_unit_ptr,
                              const int32_t* d_unit_state, int64_t units, int reversible, int stationary, int maxiter,
                              double maxerr, int n_iterations, int max_workgroups, void* d_work, double* d_A,
                              double* d_B, double* d_p0, double* d_pi, double* d_gamma, double* d_C, double* d_E,
                              double* d_gamma0, double* d_logL, double* d_history, int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_model(ctx, "msm_hmm_iterations", n, k);
    if (rs != MSM_OK) return rs;
    rs = check_tables(ctx, "msm_hmm_iterations", N, Q, n_chunks, max_workgroups);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, n_iterations >= 1 && units >= 0 && units <= N + k && maxiter >= 1 &&
                         maxiter <= MSM_HMM_MAX_FIXED_POINT && maxerr >= 0.0,
                "msm_hmm_iterations: need n_iterations >= 1, 0 <= units <= N + k, 1 <= maxiter <= %d, maxerr >= 0",
                MSM_HMM_MAX_FIXED_POINT);
    MSM_REQUIRE(ctx, d_labels && d_seq && d_chunk_ptr && (d_chunk_seq || n_chunks == 0) && d_offsets && d_members &&
                         d_unit_ptr && (d_unit_state || units == 0) && d_work && d_A && d_B && d_p0 && d_pi && d_gamma &&
                         d_C && d_E && d_gamma0 && d_logL && d_history && d_status, "msm_hmm_iterations: NULL pointer");
    const Tables tb{d_labels, N, k, n, d_seq, Q, d_chunk_ptr, d_chunk_seq, n_chunks};
    const Work w = carve(d_work, n, n_chunks, Q, units);
    for (int it = 0; it < n_iterations; ++it) {
        rs = estep_dispatch(ctx, tb, d_A, d_B, d_p0, max_workgroups, w, d_gamma, d_C, d_gamma0, d_logL, d_history + it,
                            d_status);
        if (rs != MSM_OK) return rs;
        rs = emissions_launch(ctx, d_gamma, N, n, k, d_offsets, d_members, d_unit_ptr, d_unit_state, units,
                              max_workgroups, w.Epart, d_E);
        if (rs != MSM_OK) return rs;
        hipLaunchKernelGGL(hmm_mstep_kernel, dim3(1), dim3(kFoldT), 0, ctx->stream, n, k, Q, (const double*)d_C,
                           (const double*)d_E, (const double*)d_gamma0, reversible, stationary, maxiter, maxerr, d_A,
                           d_B, d_p0, d_pi, d_status);
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
