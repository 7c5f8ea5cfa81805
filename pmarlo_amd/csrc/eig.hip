// Dense symmetric eigensolver (parallel cyclic Jacobi, one workgroup) and the
// TICA solve built on it.  Up to F = 256 the matrices are small: this stage is
// latency-bound, not bandwidth- or flop-bound, so the design
// goal is "stay on the device, one launch": no host round trip sits between
// the covariance pass and the projection pass.  Orders 257 .. 2048 are spread over
// the whole device instead (block Jacobi, eig_large.h); the three entries at the end
// of this file dispatch on the order.
//
// Jacobi: the n(n-1)/2 pivots of a sweep are visited in n-1 rounds of n/2
// disjoint pairs (round-robin tournament).  Within a round all rotations are
// independent: compute (c, s) per pair, rotate rows, then rotate columns of A and
// V.  A and V live in LDS (odd row stride, conflict-free column walks) whenever
// 2 n (n+1) doubles fit; otherwise in global scratch.
#include "common.h"
#include "wave.h"

// Diagnostic builds only (tools/probe/jacobi_probe.hip, tri_probe.hip): per-phase cycle stamps.  STAMP_ADD(slot, last)
// books the shader cycles since `last` into `slot`.  JSTAMP: every thread, into registers, flushed by thread 0 of
// jacobi_eigh.  TSTAMP (tridiag_eigh), KSTAMP (tica_solve_kernel), LSTAMP (inside the register phases; only with
// MSM_TRI_STAMPS_FINE): thread 0, straight into g_tri_stamps.
__device__ __forceinline__ unsigned long long stamp_clock() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
#define STAMP_ADD(slot, last) do { const unsigned long long t__ = stamp_clock(); slot += t__ - last; last = t__; } while (0)
#ifdef MSM_JACOBI_STAMPS
__device__ unsigned long long g_jacobi_stamps[8];
#define JSTAMP(i) STAMP_ADD(acc__[i], last__)
#define JSTAMP_INIT unsigned long long acc__[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long last__ = stamp_clock();
#define JSTAMP_FLUSH if (threadIdx.x == 0) { for (int i__ = 0; i__ < 8; ++i__) g_jacobi_stamps[i__] += acc__[i__]; }
#else
#define JSTAMP(i)
#define JSTAMP_INIT
#define JSTAMP_FLUSH
#endif
#ifdef MSM_TRI_STAMPS
__device__ unsigned long long g_tri_stamps[24];
#define TSTAMP(i) do { if (threadIdx.x == 0) STAMP_ADD(g_tri_stamps[i], tlast__); } while (0)
#define TSTAMP_INIT unsigned long long tlast__ = 0; if (threadIdx.x == 0) tlast__ = stamp_clock();
#define KSTAMP(i) do { if (threadIdx.x == 0) STAMP_ADD(g_tri_stamps[i], klast__); } while (0)
#define KSTAMP_INIT unsigned long long klast__ = 0; if (threadIdx.x == 0) klast__ = stamp_clock();
#else
#define TSTAMP(i)
#define TSTAMP_INIT
#define KSTAMP(i)
#define KSTAMP_INIT
#endif
#ifdef MSM_TRI_STAMPS_FINE
#define LSTAMP(i) TSTAMP(i)
#define LSTAMP_INIT TSTAMP_INIT
#else
#define LSTAMP(i)
#define LSTAMP_INIT
#endif

namespace {

constexpr int kEigThreads = 1024;
constexpr int kMaxPairs = 128;  // n <= 256

struct JacobiShared {
    double2 cs[kMaxPairs];  // (c, s) of pivot i: one 16-byte LDS read
    int p[kMaxPairs], q[kMaxPairs];
    int reserved[2 * kMaxPairs];  // unused: keeps sizeof (the LDS boundaries in tests/_eig_ref.py); goes only in a change that may move them
    // tables of the pipelined path (n <= 64), two buffers: colw2 = p | q << 16, roww2 = p * ld | (q * ld) << 16 (one
    // read instead of the tournament arithmetic and the row multiplies); rotations of round r+1 are formed by wave 0
    // while the other waves still apply round r
    double2 cs2[2][32];
    int colw2[2][32], roww2[2][32];
    double red[kEigThreads / 64];
    double bc[4];
    int ibc[4];
};

// Short-latency fp64 reciprocal / reciprocal square root: hardware seed plus two
// Newton steps (the IEEE division / sqrt expansions are 3-4x longer dependent chains,
// and the rotation set-up is the serial part of every Jacobi round).
__device__ __forceinline__ double nr_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(r, fma(-x, r, 1.0), r);
    r = fma(r, fma(-x, r, 1.0), r);
    return r;
}
__device__ __forceinline__ double nr_rsqrt(double x) {
    double r = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    r = r * fma(-h * r, r, 1.5);
    r = r * fma(-h * r, r, 1.5);
    return r;
}

// Jacobi rotation annihilating a_pq:  t = sgn(a) b / (|a| + sqrt(a^2 + b^2)) with
// a = (a_qq - a_pp)/2, b = a_pq;  c = 1/sqrt(1 + t^2), s = t c  (so c^2 + s^2 = 1 to
// rounding, which is what keeps V orthogonal).
__device__ __forceinline__ void jacobi_rotation(double app, double aqq, double apq, double& c, double& s) {
    c = 1.0; s = 0.0;
    if (apq == 0.0) return;
    const double a = 0.5 * (aqq - app);
    const double h2 = fma(a, a, apq * apq);
    if (!(h2 > 1e-300) || !(h2 < 1e300)) return;  // degenerate scale: skip this pivot
    // h and 1/(|a|+h) only steer the angle: one Newton step (~1e-13 relative) is plenty, the
    // pivot is zeroed explicitly; c below carries orthogonality and gets the full two steps.
    double rh = __builtin_amdgcn_rsq(h2);
    rh = rh * fma(-0.5 * h2 * rh, rh, 1.5);
    const double h = h2 * rh;
    const double den = fabs(a) + h;
    double rd = __builtin_amdgcn_rcp(den);
    rd = fma(rd, fma(-den, rd, 1.0), rd);
    const double t = (a >= 0.0 ? apq : -apq) * rd;
    c = nr_rsqrt(fma(t, t, 1.0));
    s = t * c;
}

// Round-robin tournament: pivot i of round r pairs indices (p, q); index npad-1 is the
// padding player when n is odd (it only ever appears as q).  Pure integer arithmetic (cheaper than an LDS table: the
// update phase is bound by LDS instruction issue).
// (p, q) is NOT ordered: p = round + i and q = round - i (mod npad-1) are runs of consecutive
// indices over i, so a wave's column accesses A[.][p_i] / A[.][q_i] fall on consecutive LDS
// banks (ordering the pair by min/max scrambled them: bank conflicts in the update phase).
__device__ __forceinline__ void pivot_pair(int round, int i, int npad, int& p, int& q) {
    if (i == 0) { p = round; q = npad - 1; return; }
    p = round + i; if (p >= npad - 1) p -= npad - 1;
    q = round - i; if (q < 0) q += npad - 1;
}

// (xp, xq) <- (c xp - s xq, s xp + c xq): one row of V J, or one column / row of a one-sided block update
__device__ __forceinline__ void rotate_pair(double c, double s, double& xp, double& xq) {
    const double yp = fma(-s, xq, c * xp), yq = fma(s, xp, c * xq);
    xp = yp; xq = yq;
}

// One 2x2 block of A <- J'AJ: rows p, q of pivot a (ca, sa) crossed with columns p, q of pivot b (cb, sb).  Values
// in, values out: the fast paths issue all their loads (clamped addresses) before and only predicate the stores.
__device__ __forceinline__ void rotate_block(double app, double apq, double aqp, double aqq, double ca, double sa,
                                             double cb, double sb, bool diagonal, double& npp, double& npq,
                                             double& nqp, double& nqq) {
    const double rpp = fma(-sa, aqp, ca * app), rpq = fma(-sa, aqq, ca * apq);
    const double rqp = fma(sa, app, ca * aqp), rqq = fma(sa, apq, ca * aqq);
    npp = fma(-sb, rpq, cb * rpp); npq = fma(sb, rpp, cb * rpq);
    nqp = fma(-sb, rqq, cb * rqp); nqq = fma(sb, rqp, cb * rqq);
    if (diagonal) { npq = 0.0; nqp = 0.0; }  // the pivot is annihilated exactly
}

__device__ __forceinline__ void set_identity(double* V, int n, int ld) {   // no barrier
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) V[(i / n) * ld + (i % n)] = (i / n == i % n) ? 1.0 : 0.0;
}

// Convergence test of a sweep (uniform): ||off||_F <= n*eps*||A||_F.  Rounding of the rotations themselves
// re-pollutes the zeroed entries at that level, and the eigenvalue error left is second order in it.
__device__ __forceinline__ bool jacobi_converged(const double* A, int n, int ld, JacobiShared* sh) {
    double off = 0.0, dia = 0.0;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) {
        const int r = i / n, c = i - r * n;
        const double v = A[r * ld + c];
        if (r == c) dia = fma(v, v, dia); else off = fma(v, v, off);
    }
    off = block_sum_bcast(off, sh->red, sh->bc);
    dia = block_sum_bcast(dia, sh->red, sh->bc);
    const double tol = (double)n * 2.220446049250313e-16;
    return off <= tol * tol * (dia + off) || off == 0.0;
}

// A (n x n, row stride ld, symmetric) -> diagonal; V -> eigenvectors in columns.
// Returns the number of sweeps used (uniform across the block).
//
// One round = two phases, two barriers:
//  (1) lane i of the first waves forms the rotation of pivot i -- all m = n/2 serial
//      fp64 chains of the round run side by side (a lone dependent fp64 op costs ~44
//      cycles on this chip, so the chain, not the flop count, sets the pace);
//  (2) A <- J'AJ in ONE pass: the pivots partition the indices, so A splits into m x m
//      disjoint 2x2 blocks (rows of pivot a, columns of pivot b) and block (a, b) needs
//      only its own four entries and the two rotations -- no intermediate "rows done"
//      barrier.  V <- VJ rides in the same phase.
__device__ __forceinline__ int jacobi_eigh_pipelined(double* A, double* V, int n, int ld, JacobiShared* sh,
                                                     int max_sweeps);

__device__ __forceinline__ int jacobi_eigh(double* A, double* V, int n, int ld, JacobiShared* sh, int max_sweeps) {
    const int tid = threadIdx.x, nt = blockDim.x;
    {
        const int mh = n / 2;
        if ((n & 1) == 0 && mh >= 4 && mh <= 32 && mh * mh <= nt && mh * n <= 2 * nt && n * ld < 65536 && nt >= 64)
            return jacobi_eigh_pipelined(A, V, n, ld, sh, max_sweeps);
    }
    set_identity(V, n, ld);
    __syncthreads();
    if (n < 2) return 0;
    const int npad = n + (n & 1);
    const int m = npad / 2;
    int sweep = 0;
    JSTAMP_INIT
    for (; sweep < max_sweeps; ++sweep) {
        JSTAMP(0);
        if (jacobi_converged(A, n, ld, sh)) break;
        JSTAMP(1);
        // fast path: one 2x2 block and at most two V items per thread, indices fixed for the sweep.  With 1024 threads:
        // the odd orders up to 63 and n = 2, 4, 6 (the other even orders up to 64 are pipelined)
        const bool fast = (m * m <= nt) && (m * n <= 2 * nt);
        const int my_ia = tid / m, my_ib = tid - my_ia * m;
        const bool has_blk = tid < m * m;
        const int v_ib0 = tid / n, v_r0 = tid - v_ib0 * n;
        const int v_ib1 = (tid + nt) / n, v_r1 = (tid + nt) - v_ib1 * n;
        const bool has_v0 = tid < m * n, has_v1 = tid + nt < m * n;
        // clamped copies keep every fast-path load in range for the threads without work
        const int my_ia_c = has_blk ? my_ia : 0, my_ib_c = has_blk ? my_ib : 0;
        const int v_ib0_c = has_v0 ? v_ib0 : 0, v_ib1_c = has_v1 ? v_ib1 : 0;
        const int v_r1_c = has_v1 ? v_r1 : 0;
        for (int round = 0; round < npad - 1; ++round) {
            if (tid < m) {
                const int i = tid;
                int p, q;
                pivot_pair(round, i, npad, p, q);
                double c = 1.0, s = 0.0;
                if (q < n) jacobi_rotation(A[p * ld + p], A[q * ld + q], A[p * ld + q], c, s);
                sh->cs[i] = make_double2(c, s); sh->p[i] = p; sh->q[i] = q;
            }
            JSTAMP(2);
            __syncthreads();
            JSTAMP(3);
            if (fast) {
                // Branch-free: every load uses an in-range (clamped) address and is issued
                // before the first use; only the stores are predicated.  (Predicated LOADS
                // made the compiler fence each one with s_waitcnt: ~20 exposed LDS latencies.)
                int pa, qa, pb, qb, vp0, vq0, vp1, vq1;
                pivot_pair(round, my_ia_c, npad, pa, qa);
                pivot_pair(round, my_ib_c, npad, pb, qb);
                pivot_pair(round, v_ib0_c, npad, vp0, vq0);
                pivot_pair(round, v_ib1_c, npad, vp1, vq1);
                const bool row_real = qa < n, col_real = qb < n, v0 = has_v0 && vq0 < n, v1 = has_v1 && vq1 < n;
                const int qa_c = row_real ? qa : pa, qb_c = col_real ? qb : pb;
                const int vq0_c = vq0 < n ? vq0 : vp0, vq1_c = vq1 < n ? vq1 : vp1;
                const double2 ra = sh->cs[my_ia_c], rb = sh->cs[my_ib_c], r0 = sh->cs[v_ib0_c], r1 = sh->cs[v_ib1_c];
                const double app = A[pa * ld + pb], apq = A[pa * ld + qb_c];
                const double aqp = A[qa_c * ld + pb], aqq = A[qa_c * ld + qb_c];
                double x0p = V[v_r0 * ld + vp0], x0q = V[v_r0 * ld + vq0_c];
                double x1p = V[v_r1_c * ld + vp1], x1q = V[v_r1_c * ld + vq1_c];
                // the index sitting out (odd n) is not rotated
                const double ca = row_real ? ra.x : 1.0, sa = row_real ? ra.y : 0.0;
                const double cb = col_real ? rb.x : 1.0, sb = col_real ? rb.y : 0.0;
                double npp, npq, nqp, nqq;
                rotate_block(app, apq, aqp, aqq, ca, sa, cb, sb, my_ia_c == my_ib_c, npp, npq, nqp, nqq);
                rotate_pair(r0.x, r0.y, x0p, x0q);
                rotate_pair(r1.x, r1.y, x1p, x1q);
                if (has_blk) A[pa * ld + pb] = npp;
                if (has_blk && col_real) A[pa * ld + qb] = npq;
                if (has_blk && row_real) A[qa * ld + pb] = nqp;
                if (has_blk && row_real && col_real) A[qa * ld + qb] = nqq;
                if (v0) { V[v_r0 * ld + vp0] = x0p; V[v_r0 * ld + vq0] = x0q; }
                if (v1) { V[v_r1_c * ld + vp1] = x1p; V[v_r1_c * ld + vq1] = x1q; }
                JSTAMP(4);
                JSTAMP(5);
            } else {
                for (int blk = tid; blk < m * m; blk += nt) {
                    const int ia = blk / m, ib = blk - ia * m;
                    const int pa = sh->p[ia], qa = sh->q[ia], pb = sh->p[ib], qb = sh->q[ib];
                    const bool row_real = qa < n, col_real = qb < n;  // odd n: one index sits out each round
                    if (!row_real && !col_real) continue;
                    const double ca = sh->cs[ia].x, sa = sh->cs[ia].y, cb = sh->cs[ib].x, sb = sh->cs[ib].y;
                    if (!col_real) {          // unpaired column pb: rows of pivot a only
                        double ap = A[pa * ld + pb], aq = A[qa * ld + pb];
                        rotate_pair(ca, sa, ap, aq);
                        A[pa * ld + pb] = ap; A[qa * ld + pb] = aq;
                        continue;
                    }
                    if (!row_real) {          // unpaired row pa: columns of pivot b only
                        double ap = A[pa * ld + pb], aq = A[pa * ld + qb];
                        rotate_pair(cb, sb, ap, aq);
                        A[pa * ld + pb] = ap; A[pa * ld + qb] = aq;
                        continue;
                    }
                    const double app = A[pa * ld + pb], apq = A[pa * ld + qb];
                    const double aqp = A[qa * ld + pb], aqq = A[qa * ld + qb];
                    double npp, npq, nqp, nqq;
                    rotate_block(app, apq, aqp, aqq, ca, sa, cb, sb, ia == ib, npp, npq, nqp, nqq);
                    A[pa * ld + pb] = npp; A[pa * ld + qb] = npq;
                    A[qa * ld + pb] = nqp; A[qa * ld + qb] = nqq;
                }
                JSTAMP(4);
                for (int e = tid; e < m * n; e += nt) {
                    const int ib = e / n, r = e - ib * n;
                    const int pb = sh->p[ib], qb = sh->q[ib];
                    if (qb >= n) continue;
                    const double cb = sh->cs[ib].x, sb = sh->cs[ib].y;
                    double vp = V[r * ld + pb], vq = V[r * ld + qb];
                    rotate_pair(cb, sb, vp, vq);
                    V[r * ld + pb] = vp; V[r * ld + qb] = vq;
                }
                JSTAMP(5);
            }
            __syncthreads();
            JSTAMP(6);
        }
    }
    JSTAMP_FLUSH
    return sweep;
}

// Pipelined variant for even n <= 64 (m = n/2 pivots, 2m <= 64 lanes of wave 0).
//
// In pair-index space the entries the NEXT round's rotations need sit in a fixed set of 2m
// blocks: the m diagonal blocks (all diagonal entries) and, for next pivot j, block
// (j+1, j-1) (block (1,0) for j = 0, (2,0) for j = 1, (m-1, m-2) for j = m-1) -- the
// tournament only rotates the ring.  Wave 0 updates exactly those blocks first, reads its own
// results back (LDS operations of one wave execute in order) and forms the rotations of round
// r+1 into the other table while waves 1.. apply round r to the remaining blocks and to V:
// the ~700-cycle serial rotation chain leaves the critical path and one of the two barriers
// per round goes away.
__device__ __forceinline__ int jacobi_eigh_pipelined(double* A, double* V, int n, int ld, JacobiShared* sh,
                                                     int max_sweeps) {
    const int tid = threadIdx.x, nt = blockDim.x;
    set_identity(V, n, ld);
    const int m = n / 2, ring = n - 1;
    auto form_rotations = [&](int round, int buf) {  // lanes 0..m-1 of wave 0
        int p, q;
        pivot_pair(round, tid, n, p, q);
        double c, s;
        jacobi_rotation(A[p * ld + p], A[q * ld + q], A[p * ld + q], c, s);
        sh->cs2[buf][tid] = make_double2(c, s);
        sh->colw2[buf][tid] = p | (q << 16);
        sh->roww2[buf][tid] = (p * ld) | ((q * ld) << 16);
    };
    auto update_block = [&](int ia, int ib, int buf, bool live) {
        const int wr = sh->roww2[buf][ia], wc = sh->colw2[buf][ib];
        const double2 ra = sh->cs2[buf][ia], rb = sh->cs2[buf][ib];
        double* Ap = A + (wr & 0xffff);
        double* Aq = A + (wr >> 16);
        const int pb = wc & 0xffff, qb = wc >> 16;
        const double app = Ap[pb], apq = Ap[qb], aqp = Aq[pb], aqq = Aq[qb];
        double npp, npq, nqp, nqq;
        rotate_block(app, apq, aqp, aqq, ra.x, ra.y, rb.x, rb.y, ia == ib, npp, npq, nqp, nqq);
        if (live) { Ap[pb] = npp; Ap[qb] = npq; Aq[pb] = nqp; Aq[qb] = nqq; }
    };
    // static roles
    const int my_ia = tid / m, my_ib = tid - my_ia * m;
    const bool priority = (my_ib == my_ia) || (my_ia >= 2 && my_ib == my_ia - 2) || (my_ia == 1 && my_ib == 0) ||
                          (my_ia == m - 1 && my_ib == m - 2);
    const bool has_blk = tid < m * m && !priority;
    const int my_ia_c = tid < m * m ? my_ia : 0, my_ib_c = tid < m * m ? my_ib : 0;
    // wave 0: lane l < m -> diagonal block l; lane m + j -> the block holding next pivot j
    int pr_ia = 0, pr_ib = 0;
    const bool has_pr = tid < 2 * m;
    if (tid < m) { pr_ia = tid; pr_ib = tid; }
    else if (tid < 2 * m) {
        const int j = tid - m;
        if (j == 0) { pr_ia = 1; pr_ib = 0; }
        else if (j == 1) { pr_ia = 2; pr_ib = 0; }
        else if (j == m - 1) { pr_ia = m - 1; pr_ib = m - 2; }
        else { pr_ia = j + 1; pr_ib = j - 1; }
    }
    const int v_ib0 = tid / n, v_r0 = tid - v_ib0 * n;
    const int v_ib1 = (tid + nt) / n, v_r1 = (tid + nt) - v_ib1 * n;
    const bool has_v0 = tid < m * n, has_v1 = tid + nt < m * n;
    const int v_ib0_c = has_v0 ? v_ib0 : 0, v_ib1_c = has_v1 ? v_ib1 : 0, v_r1_c = has_v1 ? v_r1 : 0;
    __syncthreads();
    int buf = 0, round = 0;
    if (tid < m) form_rotations(0, 0);
    __syncthreads();
    int sweep = 0;
    for (; sweep < max_sweeps; ++sweep) {
        if (jacobi_converged(A, n, ld, sh)) break;
        for (int rr = 0; rr < ring; ++rr) {
            const int next_round = round + 1 == ring ? 0 : round + 1;
            if (tid < 64) {  // wave 0 (uniform branch)
                update_block(pr_ia, pr_ib, buf, has_pr);
                if (tid < m) form_rotations(next_round, buf ^ 1);
            }
            update_block(my_ia_c, my_ib_c, buf, has_blk);
            {
                const int w0 = sh->colw2[buf][v_ib0_c], w1 = sh->colw2[buf][v_ib1_c];
                const double2 r0 = sh->cs2[buf][v_ib0_c], r1 = sh->cs2[buf][v_ib1_c];
                double* V0 = V + v_r0 * ld;
                double* V1 = V + v_r1_c * ld;
                const int vp0 = w0 & 0xffff, vq0 = w0 >> 16, vp1 = w1 & 0xffff, vq1 = w1 >> 16;
                double x0p = V0[vp0], x0q = V0[vq0], x1p = V1[vp1], x1q = V1[vq1];
                rotate_pair(r0.x, r0.y, x0p, x0q);
                rotate_pair(r1.x, r1.y, x1p, x1q);
                if (has_v0) { V0[vp0] = x0p; V0[vq0] = x0q; }
                if (has_v1) { V1[vp1] = x1p; V1[vq1] = x1q; }
            }
            __syncthreads();
            buf ^= 1;
            round = next_round;
        }
    }
    return sweep;
}

// order[j] = index of the j-th largest |ev| (stable; rank_order: wave.h)
__device__ void sort_desc_abs(const double* ev, int n, int* order) {
    rank_order<true>(n, order, [&](int i) { return fabs(ev[i]); });
    __syncthreads();
}

// column j of M (n rows, stride ld) *= sign of its largest-magnitude entry (first occurrence)
__device__ void canonical_signs(double* M, int n, int ncols, int ld) {
    for (int j = threadIdx.x; j < ncols; j += blockDim.x) {
        double best = -1.0, sgn = 1.0;
        for (int i = 0; i < n; ++i) {
            const double v = M[i * ld + j];
            if (fabs(v) > best) { best = fabs(v); sgn = v < 0.0 ? -1.0 : 1.0; }
        }
        if (sgn < 0.0)
            for (int i = 0; i < n; ++i) M[i * ld + j] = -M[i * ld + j];
    }
    __syncthreads();
}

// Two factorisations in lockstep (same barriers): P = chol(Mp) is only a positive-definiteness
// probe, Q = chol(Mq) is the factor that is used.  Returns false as soon as Mp loses a pivot
// (Mq is then unfinished and must not be used).
__device__ bool cholesky_lower_pair(double* Mp, double* Mq, int n, int ld, JacobiShared* sh) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int j = 0; j < n; ++j) {
        if (tid < 2) {
            double* M = tid == 0 ? Mp : Mq;
            const double dj = M[j * ld + j];
            sh->ibc[1 + tid] = dj > 0.0 ? 1 : 0;
            if (dj > 0.0) M[j * ld + j] = sqrt(dj);
        }
        __syncthreads();
        if (!sh->ibc[1] || !sh->ibc[2]) return false;
        const double pjj = Mp[j * ld + j], qjj = Mq[j * ld + j];
        for (int i = j + 1 + tid; i < n; i += nt) {
            Mp[i * ld + j] /= pjj;
            Mq[i * ld + j] /= qjj;
        }
        __syncthreads();
        const int m = n - j - 1;
        for (int e = tid; e < m * m; e += nt) {
            const int a = e / m, b = e - a * m;  // trailing (j+1+a, j+1+b), lower part only
            if (b <= a) {
                const int ra = (j + 1 + a) * ld, rb = (j + 1 + b) * ld;
                Mp[ra + j + 1 + b] -= Mp[ra + j] * Mp[rb + j];
                Mq[ra + j + 1 + b] -= Mq[ra + j] * Mq[rb + j];
            }
        }
        __syncthreads();
    }
    return true;
}

// X = G^-1 for lower-triangular G; X lower.  Right-looking elimination on [G | I]: per pivot k
// one scaling of row k and one rank-1 update of the rows below, both fully parallel -- n short
// steps instead of per-column chains of ~n^2/2 dependent FMAs (a dependent fp64 FMA costs ~44
// cycles here, a workgroup barrier ~100).  X must not alias G.
__device__ void lower_inverse(const double* G, double* X, int n, int ld) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, c = e - i * n;
        X[i * ld + c] = i == c ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        const double gkk = G[k * ld + k];
        for (int c = tid; c <= k; c += nt) X[k * ld + c] /= gkk;
        __syncthreads();
        const int rows = n - k - 1, cols = k + 1;
        for (int e = tid; e < rows * cols; e += nt) {
            const int a = e / cols, c = e - a * cols;
            const int i = k + 1 + a;
            X[i * ld + c] = fma(-G[i * ld + k], X[k * ld + c], X[i * ld + c]);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// Symmetric eigensolver for n <= 64 without the ~600 barrier-bound Jacobi rounds:
//   (1) Householder tridiagonalisation A = Q T Q' with A and Q' held in the registers of eight waves (householder_phase
//       below: rows dealt out four ways, lane = column, two barriers per column);
//   (2) all eigenvalues of T at once by multisection on Sturm counts: 8 lanes per eigenvalue (two waves per SIMD: a
//       lone wave only gets every other issue slot), 8 trial points per round, 20 rounds; the count uses the product
//       recurrence p_j = (d_j - x) p_{j-1} - e_{j-1}^2 p_{j-2} (no division), sign changes shifted into a bit mask,
//       rescaled every 8 rows;
//   (3) one eigenvector of T per lane from the twisted factorisation of T - lambda I (forward and backward
//       pivots, twist at the smallest |gamma|: Parlett & Dhillon), i.e. one exact inverse-iteration step;
//   (4) Z = Q X on the matrix cores, the 1/|x| factors folded into the operand.
// Eigenvectors of T belonging to eigenvalues closer than ~1e-9 |T| come out of (3) short of orthogonal, and
// exactly repeated eigenvalues give repeated vectors: X'X is checked and the caller falls back to Jacobi on its
// copy of A when the defect exceeds `orth_tol` (or a residual |T x - lambda x| is large).
// ---------------------------------------------------------------------------------------------------
constexpr int kTriMax = 64;
constexpr int kTriLd = 65;   // row stride of every matrix handed to tridiag_eigh (a constant: row offsets become immediates)
struct TriShared {
    double2 de[kTriMax + 8];   // {d_j, e_{j-1}^2} of the scaled matrix; rows n.. are {8, 0} (no sign change)
    double d[kTriMax], e[kTriMax], lam[kTriMax], praw[kTriMax], uq[kTriMax], inv[kTriMax];
    double scale, gl, gu;
    double red[kEigThreads / 64];
    int bad;
    double part[16][kTriMax];  // partial products of the tridiagonalisation, one row per wave (the LDL' phase keeps its pivot rows there)
    union {                    // the two register-resident phases never overlap
        double2 vw[8][kTriMax];                 // tridiagonalisation: {v_j, w_j} of the column in flight, one copy per A wave
        alignas(16) double lv[16][kTriMax];     // unused since the LDL' phase went to the matrix cores: keeps sizeof (tests/_eig_ref.py)
    };
    double vpub[2][kTriMax];   // tridiagonalisation: the reflector of column k for the Q' waves, slot k & 1
    double taupub[2];
};

// C[i][j] = sum_k opA(i,k) opB(k,j) on the matrix cores (v_mfma_f64_16x16x4_f64; one 16 x 16 tile of C per wave
// and trip), i < rows, j < cols, k < inner; opA = A or A', opB = B or B'.  bscale (optional) multiplies column j of
// opB.  C must not alias A or B.  A 64^3 product costs what it costs on the VALU (the fp64 rates are equal) but
// reads each operand from the LDS once per tile instead of once per multiply.  One tile: mfma_tile_acc (wave.h).
template <bool TA, bool TB>
__device__ __forceinline__ void mfma_mm(double* C, const double* A, const double* B, int rows, int cols, int inner, int ld,
                        const double* bscale = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int tr = (rows + 15) >> 4, tc = (cols + 15) >> 4;
    for (int t = wave; t < tr * tc; t += nw) {
        const int i0 = (t / tc) * 16, c0 = (t - (t / tc) * tc) * 16;
        const bool aok = i0 + j < rows, bok = c0 + j < cols;
        const int ai = aok ? i0 + j : 0, bj = bok ? c0 + j : 0;
        const double bs = bscale ? bscale[bj] : 1.0;
        const v4f64 acc = mfma_tile_acc(
            inner, g, aok, bok, [&](int k) { return TA ? A[k * ld + ai] : A[ai * ld + k]; },
            [&](int k) { return (TB ? B[bj * ld + k] : B[k * ld + bj]) * bs; });
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + g + 4 * r, col = c0 + j;
            if (row < rows && col < cols) C[row * ld + col] = acc[r];
        }
    }
    __syncthreads();
}

// # eigenvalues of the (scaled) tridiagonal matrix below x: sign changes of p_{-1} = 1, p_0, ..., p_{n-1}.  The sign
// bits are shifted into a mask as the rows go by (one v_alignbit per row) and the changes counted at the end,
// popc(S ^ (S >> 1)) per 32 rows: per row 4 vector instructions (sub, mul, fma, alignbit).  An exact zero counts as
// positive: it only occurs when x is an eigenvalue of a leading block, and a bracket spoilt by it fails the residual
// check.  Eight rows at a time: their {d, e^2} pairs come out of the LDS in one burst.
__device__ __forceinline__ int sturm_count(const TriShared* ts, int nblocks, double x) {
    double pp = 0.0, p = 1.0;
    unsigned bits = 0, w0 = 0;
    for (int b = 0; b < nblocks; ++b) {
        // the rows are re-read from the LDS on every call: kept in registers across the rounds of the caller they
        // would take 2 x 128 registers, and the compiler spills to scratch to try
        asm volatile("" ::: "memory");
        double2 r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = ts->de[8 * b + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double pn = fma(r[u].x - x, p, -(r[u].y * pp));
            bits = __builtin_amdgcn_alignbit(bits, (unsigned)__double2hiint(pn), 31);   // (bits << 1) | sign(pn)
            pp = p;
            p = pn;
        }
        if (b & 1) {
            // keep the pair in range: the matrix is scaled to |T| <= 1, so sixteen rows grow it by 2.5^16 at most and
            // cannot shrink it below the normal range unless x sits within 1e-19 of sixteen diagonal entries in a row
            const int ex = max(__builtin_amdgcn_frexp_exp(p), __builtin_amdgcn_frexp_exp(pp));
            p = ldexp(p, -ex);
            pp = ldexp(pp, -ex);
        }
        if (b == 3) { w0 = bits; bits = 0; }
    }
    if (nblocks <= 4) return __popc(bits ^ (bits >> 1));   // right-aligned: the zeros above stand for p_{-1} > 0
    // rows 32.. sit right-aligned in `bits`; the row above the first of them is row 31 = bit 0 of w0
    const int r1 = 8 * nblocks - 32;
    return __popc(w0 ^ (w0 >> 1)) + __popc(bits ^ ((bits >> 1) | ((w0 & 1u) << (r1 - 1))));
}

// Tridiagonalisation A = Q T Q' with the matrices held in REGISTERS, every wave of the workgroup at work, two
// barriers per column.
// Measured on this chip (tools/probe/lone_wave_lds_probe.hip, tri_probe.hip): a wave issues about one instruction per
// 10 cycles whatever the instruction and however many waves share its SIMD (a SIMD takes one per ~4 cycles between
// all its waves), pays ~37 cycles per taken branch and 12-19 per LDS instruction, so one barrier-free wave sweeping an
// LDS-resident matrix needed ~5000 cycles per column and sixteen waves sweeping it between barriers were no faster.
// Here nothing is swept and the per-wave instruction chain of a column is kept short:
//   waves 0-7 hold the rows j = w (mod 8) of A for the whole reduction, waves 8-15 the same rows of Q'
//   (QT[j][r] = Q[r][j]): 8 doubles per lane, indexed by compile-time constants only (lane = column);
//   A waves, column k (the reflector of column 0 is formed ahead of the loop):
//   (1) partial product p = A22 v over the own rows (the v_j come back as broadcast reads of the wave's own LDS copy);
//       barrier 1;
//   (2) the eight partials are summed in a fixed order, w = tau p - (tau^2 p.v / 2) v; the owner of row k + 1 puts the
//       new value of that row in the LDS at once; barrier 2;
//   (3) a_j -= v_j w + w_j v on the own rows and, in the same straight-line stretch, the reflector of column k + 1
//       from row k + 1, every A wave for itself (same inputs, same instructions, same bits): x = A[k+1][k+2:],
//       H = I - tau v v', v_{k+2} = 1; wave 0 also leaves v and tau in the LDS for the Q' waves.  A column that is
//       already reduced gives tau = 0 and everything downstream of it is arithmetic with zeros: no branches.
//   Q' waves run half a column behind and never form a reflector: between barrier 1 and 2 of column k they read v_k and
//   write their partial u = Q v; between barrier 2 and barrier 1 of the next column they sum the partials and apply
//   q_j -= tau v_j u.  They add nothing to the A waves' chain, which is what a column costs.
// Rows up to k carry v_j = w_j = 0; groups of four own rows that lie entirely there are skipped.
template <typename F>
__device__ __forceinline__ void hh_for_groups(int sub, int k, F&& body) {
    // own rows sub + 8 t, t = 4 g + u; group g is dead once its last row sub + 32 g + 24 <= k
#pragma unroll
    for (int g = 0; g < 2; ++g)
        if (sub + 32 * g + 24 > k) body(g);
}
__device__ __forceinline__ void householder_phase(double* A, double* QT, int n, TriShared* ts) {
    static_assert(kEigThreads == 1024, "householder_phase deals the rows of A and Q' over sixteen waves");
    constexpr int ld = kTriLd;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool in = lane < n;
    const bool is_a = wave < 8;
#ifdef MSM_TRI_NOQ   // diagnostic build only (tools/probe/tri_probe.hip): what the tridiagonalisation costs without its Q waves
    const bool is_q = false;
#else
    const bool is_q = !is_a;
#endif
    const int sub = wave & 7;
    double* part = ts->part[wave];
    const double* parts = ts->part[is_a ? 0 : 8];
    double2* vw = ts->vw[sub];        // A waves: this wave's own copy of {v_j, w_j}
    double m[8];                      // rows sub + 8 t of A or Q', column `lane`
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int j = sub + 8 * t;
        m[t] = (in && j < n) ? (is_a ? A[j * ld + lane] : (j == lane ? 1.0 : 0.0)) : 0.0;
    }
    // Q' side of column c: partial u = Q v over the own rows / sum of the partials and the update
    auto q_partial = [&](int c) {
        if (__builtin_amdgcn_readfirstlane(ts->taupub[c & 1] != 0.0)) {
            const double* vp = ts->vpub[c & 1];
            double s0 = 0.0, s1 = 0.0;
            hh_for_groups(sub, c, [&](int g) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = vp[sub + 32 * g + 8 * u];
                s0 = fma(m[4 * g], v[0], s0);
                s1 = fma(m[4 * g + 1], v[1], s1);
                s0 = fma(m[4 * g + 2], v[2], s0);
                s1 = fma(m[4 * g + 3], v[3], s1);
            });
            part[lane] = s0 + s1;
        }
    };
    auto sum_parts = [&]() {
        return (((parts[lane] + parts[kTriMax + lane]) + (parts[2 * kTriMax + lane] + parts[3 * kTriMax + lane])) +
                ((parts[4 * kTriMax + lane] + parts[5 * kTriMax + lane]) + (parts[6 * kTriMax + lane] + parts[7 * kTriMax + lane])));
    };
    auto q_finish = [&](int c) {
        const double tau_c = ts->taupub[c & 1];
        if (__builtin_amdgcn_readfirstlane(tau_c != 0.0)) {
            const double* vp = ts->vpub[c & 1];
            const double tu = -tau_c * sum_parts();
            hh_for_groups(sub, c, [&](int g) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = vp[sub + 32 * g + 8 * u];
#pragma unroll
                for (int u = 0; u < 4; ++u) m[4 * g + u] = fma(tu, v[u], m[4 * g + u]);
            });
        }
    };
    // reflector of column c from row c in the LDS (straight-line: a column that is already reduced gives tau = 0, v = e_{c+1},
    // and everything downstream of it is a no-op); wave 0 also records d_c, e_c and leaves v, tau for the Q' waves
    auto reflector = [&](int c, double& vi, double& tau) {
        const double* rowc = A + c * ld;
        double xi = rowc[in ? lane : 0];
        const double alpha = rowc[c + 1];
        if (wave == 0 && lane == c) ts->d[c] = xi;
        const bool actc = in && lane > c;
        if (!actc) xi = 0.0;
        const double sigma = wave_sum_all(lane > c + 1 ? xi * xi : 0.0);
        const bool nz = sigma != 0.0;   // the same in every lane
        const double h2 = fma(alpha, alpha, sigma);
        const double rs = nr_rsqrt(nz ? h2 : 1.0);
        const double beta = nz ? -copysign(h2 * rs, alpha) : alpha;
        tau = nz ? (beta - alpha) * -copysign(rs, alpha) : 0.0;   // (beta - alpha) / beta
        const double scal = nr_rcp(nz ? alpha - beta : 1.0);
        vi = actc ? (lane == c + 1 ? 1.0 : (nz ? xi * scal : 0.0)) : 0.0;
        if (wave == 0) {
            ts->vpub[c & 1][lane] = vi;
            if (lane == 0) { ts->e[c] = beta; ts->taupub[c & 1] = tau; }
        }
        vw[lane].x = vi;
    };
    LSTAMP_INIT
    double vi = 0.0, tau = 0.0;
    if (is_a && n > 2) reflector(0, vi, tau);
    for (int k = 0; k + 2 < n; ++k) {
        LSTAMP(16);
        const bool act = in && lane > k;
        if (is_a) {
            // partial product p = A22 v over the own rows
            double s0 = 0.0, s1 = 0.0;
            hh_for_groups(sub, k, [&](int g) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = vw[sub + 32 * g + 8 * u].x;
                s0 = fma(m[4 * g], v[0], s0);
                s1 = fma(m[4 * g + 1], v[1], s1);
                s0 = fma(m[4 * g + 2], v[2], s0);
                s1 = fma(m[4 * g + 3], v[3], s1);
            });
            part[lane] = s0 + s1;
            LSTAMP(18);
        } else if (is_q && k > 0) {
            q_finish(k - 1);
        }
        __syncthreads();
        LSTAMP(19);
        double wi = 0.0;
        if (is_a) {
            const double p = sum_parts();
            const double pv = wave_sum_all(act ? p * vi : 0.0);
            const double al = -0.5 * tau * (tau * pv);
            wi = act ? fma(tau, p, al * vi) : 0.0;
            vw[lane].y = wi;
            LSTAMP(20);
            // the owner of row k + 1 leaves its new value in the LDS ahead of the rest of the update: everybody's next
            // reflector hangs on it (the same two fmas again below: the same bits)
#pragma unroll
            for (int t2 = 0; t2 < 8; ++t2)
                if (sub + 8 * t2 == k + 1) {
                    const double2 bk = vw[k + 1];
                    if (in) A[(k + 1) * ld + lane] = fma(-wi, bk.x, fma(-vi, bk.y, m[t2]));
                }
        } else if (is_q) {
            q_partial(k);
        }
        LSTAMP(21);
        __syncthreads();
        if (is_a) {
            // rank-2 update of the own rows (rows up to k carry v_j = w_j = 0: untouched) and, in the same straight-line
            // stretch, the reflector of the next column: two independent chains for the scheduler to interleave
            double2 bb[8];
#pragma unroll
            for (int t2 = 0; t2 < 8; ++t2) bb[t2] = vw[sub + 8 * t2];
            const double vk = vi, wk = wi;
            if (k + 3 < n) reflector(k + 1, vi, tau);
#pragma unroll
            for (int t2 = 0; t2 < 8; ++t2) m[t2] = fma(-wk, bb[t2].x, fma(-vk, bb[t2].y, m[t2]));
            LSTAMP(17);
        }
    }
    if (is_q && n > 2) q_finish(n - 3);
    // back to the LDS: Q' whole, of A the last two rows (the 2 x 2 block the reduction leaves)
    if (is_q && in) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (sub + 8 * t < n) QT[(sub + 8 * t) * ld + lane] = m[t];
    }
    if (is_a && in) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (sub + 8 * t >= n - 2 && sub + 8 * t < n) A[(sub + 8 * t) * ld + lane] = m[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ts->d[n - 2] = A[(n - 2) * ld + n - 2];
        ts->e[n - 2] = A[(n - 1) * ld + n - 2];
        ts->d[n - 1] = A[(n - 1) * ld + n - 1];
        ts->e[n - 1] = 0.0;
    }
}

// Whitening of a full-rank C00: an LDL' elimination of [C00 | I] (X = L^-1 grows out of the identity), four pivots per
// barrier, both matrices in matrix-core accumulators from start to end.  Wave w holds the 16 x 16 tile (I, J) =
// (w / 4, w % 4) of C00 and the same tile of X; one v_mfma_f64_16x16x4_f64 is exactly the rank-4 update of a tile.
// Block b, pivots j0 = 4 b .. j0 + 3: the waves of the row tile that holds rows j0 .. j0 + 3 have left them in the LDS
// (entry (g + 4 r, j) of a tile sits in acc[r] of lane (j, g): the four rows are one accumulator register of the
// tile's 64 lanes).  The trailing matrix is symmetric, so those rows are also the panel's columns.  Every lane
// eliminates the four pivots one after the other, as the unblocked elimination does, on the 4 x 4 diagonal block
// (the same numbers in every lane: the pivots d_c and the multipliers among the four rows) and on the two columns
// it feeds to the matrix core: row i0 + j of the multipliers l_ic = u_c[i] / d_c, zero up to the pivot's own row so
// that finished rows stay, and column c0 + j of the eliminated pivot rows u_c of C00 and of X.  Then one instruction
// per tile, and the owners of the next four rows leave them for the next block.
// On success W = (D^-1/2 L^-1)' (upper triangular, W' C00 W = I) is written to `W`; false (uniformly) as soon as a
// pivot is not positive, whichever of a block's four it is.  C is left as it was.  blockDim.x == 1024.
// mode 1: C00 and X (the caller certifies full rank from W, see tica_solve_kernel);
// mode 2: the probe C00 - epsilon I alone, nothing is written to W.
__device__ __forceinline__ bool ldl_whiten_registers(const double* C, double* W, int n, double epsilon, TriShared* ts,
                                                     int mode) {
    static_assert(kEigThreads == 1024 && kTriMax == 64, "ldl_whiten_registers deals 4 x 4 tiles of 16 x 16 over sixteen waves");
    constexpr int ld = kTriLd;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jj = lane & 15, g = lane >> 4;
    const int I = wave >> 2, J = wave & 3, i0 = 16 * I, c0 = 16 * J;
    const bool with_x = mode == 1;
    const bool live = i0 < n && c0 < n;   // the tile holds entries of the matrix
    v4f64 ac, ax;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = i0 + g + 4 * r, col = c0 + jj;
        const bool ok = row < n && col < n;
        const double c = C[ok ? row * ld + col : 0];
        ac[r] = ok ? c - (mode == 2 && row == col ? epsilon : 0.0) : 0.0;
        ax[r] = ok && row == col ? 1.0 : 0.0;
    }
    // pivot rows of block b: part[8 (b & 1) + g] of C00, part[8 (b & 1) + 4 + g] of X
    if (I == 0) {
        ts->part[g][c0 + jj] = ac[0];
        ts->part[4 + g][c0 + jj] = ax[0];
    }
    __syncthreads();
    LSTAMP_INIT
    for (int I0 = 0; I0 < 4; ++I0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j0 = 16 * I0 + 4 * r;
            if (j0 >= n) break;   // uniform
            const double* pc = ts->part[8 * (r & 1)];   // 16 I0 + 4 r: the block's parity is r's
            const double* px = pc + 4 * kTriMax;
            // ---- the 4 x 4 diagonal block: pivots, their reciprocals, the multipliers among the four rows
            double2 blk[4][2];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int h = 0; h < 2; ++h) blk[c][h] = *reinterpret_cast<const double2*>(pc + c * kTriMax + j0 + 2 * h);
            const bool ok1 = j0 + 1 < n, ok2 = j0 + 2 < n, ok3 = j0 + 3 < n;   // pivots past n: rows of zeros, no test
            const double d0 = blk[0][0].x;
            bool bad = !(d0 > 0.0);
            const double r0 = nr_rcp(d0);
            const double l10 = blk[0][0].y * r0, l20 = blk[0][1].x * r0, l30 = blk[0][1].y * r0;
            const double b11 = fma(-l10, blk[0][0].y, blk[1][0].y), b12 = fma(-l10, blk[0][1].x, blk[1][1].x);
            const double b13 = fma(-l10, blk[0][1].y, blk[1][1].y);
            const double d1 = ok1 ? b11 : 1.0;
            bad = bad || !(d1 > 0.0);
            const double r1 = nr_rcp(d1);
            const double l21 = b12 * r1, l31 = b13 * r1;
            const double b22 = fma(-l21, b12, fma(-l20, blk[0][1].x, blk[2][1].x));
            const double b23 = fma(-l21, b13, fma(-l20, blk[0][1].y, blk[2][1].y));
            const double d2 = ok2 ? b22 : 1.0;
            bad = bad || !(d2 > 0.0);
            const double r2 = nr_rcp(d2);
            const double l32 = b23 * r2;
            const double b33 = fma(-l32, b23, fma(-l31, b13, fma(-l30, blk[0][1].y, blk[3][1].y)));
            const double d3 = ok3 ? b33 : 1.0;
            bad = bad || !(d3 > 0.0);
            const double r3 = nr_rcp(d3);
            LSTAMP(13);
            if (__builtin_amdgcn_readfirstlane((int)bad)) return false;   // the same numbers in every lane of every wave
            if (with_x && wave == 0 && lane < 4 && j0 + lane < n)
                ts->inv[j0 + lane] = nr_rsqrt(lane == 0 ? d0 : (lane == 1 ? d1 : (lane == 2 ? d2 : d3)));
            // column `col` of the four pivot rows, eliminated one after the other
            auto eliminate = [&](const double* rows, int col, double (&u)[4]) {
                const double p0 = rows[col], p1 = rows[kTriMax + col], p2 = rows[2 * kTriMax + col], p3 = rows[3 * kTriMax + col];
                u[0] = p0;
                u[1] = fma(-l10, u[0], p1);
                u[2] = fma(-l21, u[1], fma(-l20, u[0], p2));
                u[3] = fma(-l32, u[2], fma(-l31, u[1], fma(-l30, u[0], p3)));
            };
            if (live && I >= I0) {   // uniform; row tiles above the pivots are finished
                double ua[4];
                eliminate(pc, i0 + jj, ua);
                // multiplier of row i0 + jj for pivot j0 + g (zero up to the pivot's own row), pivot row g at column c0 + jj
                const double mg = g == 0 ? ua[0] * r0 : (g == 1 ? ua[1] * r1 : (g == 2 ? ua[2] * r2 : ua[3] * r3));
                const double a = i0 + jj > j0 + g ? -mg : 0.0;
                if (J >= I) {   // pivot rows are only ever read to the right of the pivot: the tiles below the diagonal are never used
                    double ub[4];
                    eliminate(pc, c0 + jj, ub);
                    const double b = g == 0 ? ub[0] : (g == 1 ? ub[1] : (g == 2 ? ub[2] : ub[3]));
                    ac = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, ac, 0, 0, 0);
                }
                if (with_x && J <= I) {   // X is lower triangular: the tiles above the diagonal stay zero
                    double ux[4];
                    eliminate(px, c0 + jj, ux);
                    const double bx = g == 0 ? ux[0] : (g == 1 ? ux[1] : (g == 2 ? ux[2] : ux[3]));
                    ax = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bx, ax, 0, 0, 0);
                }
                // the next four rows for the next block
                if (j0 + 4 < n && I == (r < 3 ? I0 : I0 + 1)) {
                    double* nc = ts->part[8 * ((r + 1) & 1)];
                    nc[g * kTriMax + c0 + jj] = ac[r < 3 ? r + 1 : 0];
                    nc[(4 + g) * kTriMax + c0 + jj] = ax[r < 3 ? r + 1 : 0];
                }
            }
            LSTAMP(14);
            __syncthreads();
            LSTAMP(15);
        }
    }
    if (with_x && live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + g + 4 * r, col = c0 + jj;
            if (row < n && col < n) W[col * ld + row] = ax[r] * ts->inv[row];   // X is lower triangular: zeros above the diagonal of W'
        }
    }
    __syncthreads();
    return true;
}

// A: symmetric n x n (destroyed; on success its columns hold the eigenvectors, ascending eigenvalues in
// ts->lam).  Q (ends up holding Q'), X: n x n work matrices (same stride).  Returns false (uniformly) when the result must not be
// used; the caller then solves its own copy of A by Jacobi.  blockDim.x == 1024.
//
// want > 0: only the `want` pairs of largest |eigenvalue| will be read (order: |ev| descending, equal ones by solver
// index, the rule of rank_order<true>; sel: an LDS array of n ints).  They lie among the want + 1 algebraically
// smallest and the want + 1 largest eigenvalues, the candidates.  Only those nc = 2 (want + 1) and one guard beyond them
// at either end are bracketed, each by the instructions and probe points the full solve spends on it, and everything
// after (twisted factorisation, acceptance test, Z = Q X) runs on the candidates' nc columns alone -- the arithmetic
// of a column does not depend on where it sits, so every number carries the bits the full solve gives it.  On return
// kept = nc, ts->lam[0 .. nc) and columns 0 .. nc - 1 of A hold the candidates by ascending solver index; ranked among
// themselves by the same rule, the first `want` are the leading pairs of the whole spectrum in their order.
// kept = 0 says that all n pairs were computed, as without `want`:
//   * when candidates and guards are all there is, 2 (want + 2) >= n;
//   * when the candidates ranked want-th and (want + 1)-th have the same |ev|: an eigenvalue outside the candidates can
//     enter the leading set only through such a tie (it has want + 1 candidates no smaller than itself on its side of
//     the spectrum, of which at most want - 1 may rank ahead of it), and then the full order decides;
//   * when a guard lies within kTriGuard (of |T| <= 1) of the candidate next to it: the two vectors would fail the
//     orthogonality test of the full solve, which this one could not see.
// Going back costs a second eigenvalue phase (about 63 k cycles, 27 us, on top of what the full solve takes): the
// phase is one dependent chain per wave, as long for the missing brackets as for all of them.
// What stays out of sight is every failed acceptance that involves a vector this solve does not form -- a residual
// of such a vector, a pair of such vectors short of orthogonal, or a candidate and a guard more than kTriGuard apart
// that still miss orth_tol: it sends the full solve to Jacobi and not this one, and the kept pairs then agree to the
// accuracy of the two solvers, not bit for bit.
// kTriGuard is an observed figure, not a bound: pairs up to ~1e-9 |T| apart are the ones seen to miss the tolerances
// (the comment above TriShared), and the guard keeps three decades from that.  The estimate n eps / gap of the
// defect of two independently computed vectors would ask for n eps / orth_tol = 1.4e-3 at n = 64, orth_tol = 1e-11,
// which neighbours in an ordinary whitened spectrum undercut while their vectors pass the test by orders of magnitude.
constexpr double kTriGuard = 1e-6;
__device__ __forceinline__ bool tridiag_eigh(double* A, double* Q, double* X, int n, int ld, TriShared* ts, double orth_tol,
                                             int want, int* sel, int& kept) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    kept = 0;
    if (n == 1) {
        if (tid == 0) { ts->lam[0] = A[0]; A[0] = 1.0; }
        __syncthreads();
        return true;
    }
    if (ld != kTriLd) return false;
    TSTAMP_INIT
    if (tid == 0) ts->bad = 0;
    __syncthreads();
    TSTAMP(0);
    // ---- (1) tridiagonalisation
    householder_phase(A, Q, n, ts);
    TSTAMP(1);
    __syncthreads();
    TSTAMP(2);
    {   // scale to |T| <= 1 by a power of two (exact), Gershgorin bounds of the scaled matrix: wave-parallel
        const double dl = lane < n ? ts->d[lane] : 0.0, el = lane < n ? ts->e[lane] : 0.0;
        double an = fmax(fabs(dl), fabs(el));
        // wave_max_xor (wave.h) written out, here and for `worst` below: as a call it changes the code of the index
        // divisions around it, and the solve is one latency-bound chain
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) an = fmax(an, __shfl_xor(an, off, 64));
        double sc = 1.0;
        if (an > 0.0 && an < 1e300) { int ex; (void)frexp(an, &ex); sc = ldexp(1.0, -ex); }
        const double ds = dl * sc, es = el * sc;
        const double em = lane > 0 && lane < n ? ts->e[lane - 1] * sc : 0.0;
        const double rad = fabs(em) + (lane + 1 < n ? fabs(es) : 0.0);
        double gl = lane < n ? ds - rad : 1e300, gu = lane < n ? ds + rad : -1e300;
        wave_minmax_xor(gl, gu);
        __syncthreads();   // every wave has read the unscaled d, e
        if (wave == 0) {
            if (lane < n) { ts->d[lane] = ds; ts->e[lane] = es; ts->de[lane] = make_double2(ds, em * em); }
            else ts->de[lane] = make_double2(8.0, 0.0);
            if (lane < 8) ts->de[kTriMax + lane] = make_double2(8.0, 0.0);
            if (lane == 0) {
                if (!(an < 1e300)) ts->bad = 1;   // NaN / inf input
                ts->scale = sc;
                const double bn = fmax(fabs(gl), fabs(gu));
                const double pad = 4.0 * n * 2.220446049250313e-16 * bn + 1e-290;
                ts->gl = gl - pad;
                ts->gu = gu + pad;
            }
        }
    }
    __syncthreads();
    TSTAMP(3);
    if (ts->bad) return false;
    // ---- (2) eigenvalues: eigenvalue i = tid / 8 is bracketed by 8 lanes (the first eight waves, two per SIMD).
    // 20 rounds: 9^20 = 2^63.4, the brackets end at rounding level (2^55.7 left 4e-12 of orthogonality defect on a
    // cond-1e4 matrix)
    // Leading pairs only: the nb = 2 (want + 2) eigenvalues at the two ends are bracketed, slot b is eigenvalue b at the
    // lower end, n - nb + b at the upper one; otherwise nb = n and slot b is eigenvalue b.  The loop runs once, or twice
    // when a tie at the cut or a close guard sends it back for all n.
    bool lead = want > 0 && 2 * (want + 2) < n;
    int nb = lead ? 2 * (want + 2) : n;
    int na = n;   // columns of X from here on
    for (;;) {
        if (tid < 8 * kTriMax && wave * 8 < nb) {
            const int b = tid >> 3, t = tid & 7;
            const int i = !lead || b < want + 2 ? b : n - nb + b;
            const int nblocks = (n + 7) >> 3;
            double lo = ts->gl, hi = ts->gu;
            const double frac = (double)(t + 1) * (1.0 / 9.0);
            for (int it = 0; it < 20; ++it) {
                const double x = fma(hi - lo, frac, lo);
                const int c = sturm_count(ts, nblocks, x);
                double nlo = c <= i ? x : lo, nhi = c > i ? x : hi;
                lo = row8_reduce(nlo, hw_max_f64);   // the 8 lanes of eigenvalue i agree on the tightest bracket
                hi = row8_reduce(nhi, hw_min_f64);
            }
            if (b < nb && t == 0) ts->lam[i] = 0.5 * (lo + hi);
        }
        __syncthreads();
        if (!lead) break;
        const int nc = 2 * (want + 1);   // candidate c is eigenvalue c (c <= want) or n - nc + c
        const auto cand = [&](int c) { return c <= want ? c : n - nc + c; };
        const auto key = [&](int c) { return fabs(ts->lam[cand(c)] / ts->scale); };   // the value the caller's sort sees
        rank_order<true>(nc, sel, key);
        __syncthreads();
        const bool lone = ts->lam[want + 1] - ts->lam[want] > kTriGuard &&
                          ts->lam[n - want - 1] - ts->lam[n - want - 2] > kTriGuard;
        if (lone && key(sel[want - 1]) != key(sel[want])) {   // uniform
            const double lk = tid < nc ? ts->lam[cand(tid)] : 0.0;   // the candidates move to the front
            __syncthreads();
            if (tid < nc) ts->lam[tid] = lk;
            __syncthreads();
            na = nc;
            break;
        }
        __syncthreads();   // sel and lam have been read: lam is written again
        lead = false;
        nb = n;
    }
    TSTAMP(4);
    // ---- (3) eigenvectors of T, column i = lane (eigenvalue i, or the i-th candidate): wave 0 runs the forward pivots
    // q_j (into X[:, i]), wave 1 the backward pivots r_j (their reciprocals into A[:, i]); gamma_j = q_j - e_j^2 / r_{j+1}
    // is smallest at the twist k; z_k = 1, z_j = -(e_j / q_j) z_{j+1} above it (wave 0), z_{j+1} = -(e_j / r_{j+1}) z_j
    // below (wave 1).
    // Every loop takes its rows eight at a time so that the LDS reads of a block are in flight together.
    const double tiny = 1e-290;
    double* Xc = X + (lane < na ? lane : 0);
    double* Ac = A + (lane < na ? lane : 0);
    const double lamb = ts->lam[lane < na ? lane : 0];
    if (wave == 0 && lane < na) {
        double q = ts->de[0].x - lamb;
        Xc[0] = q;
        for (int j0 = 1; j0 < n; j0 += 8) {
            double2 r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = ts->de[j0 + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (j0 + u < n) {
                    if (fabs(q) < tiny) q = -tiny;
                    q = fma(-r[u].y, nr_rcp(q), r[u].x - lamb);
                    Xc[(j0 + u) * ld] = q;
                }
            }
        }
    } else if (wave == 1 && lane < na) {
        double r = ts->de[n - 1].x - lamb;
        if (fabs(r) < tiny) r = -tiny;
        double ir = nr_rcp(r);
        Ac[(n - 1) * ld] = ir;
        for (int j0 = n - 2; j0 >= 0; j0 -= 8) {
            double dj[8], e2[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 - u >= 0 ? j0 - u : 0;
                dj[u] = ts->de[j].x;
                e2[u] = ts->de[j + 1].y;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (j0 - u >= 0) {
                    r = fma(-e2[u], ir, dj[u] - lamb);
                    if (fabs(r) < tiny) r = -tiny;
                    ir = nr_rcp(r);
                    Ac[(j0 - u) * ld] = ir;
                }
            }
        }
    }
    __syncthreads();
    int kk = n - 1;
    if (wave < 2 && lane < na) {
        double gbest = fabs(Xc[(n - 1) * ld]);   // gamma_{n-1} = q_{n-1}
        for (int j0 = n - 2; j0 >= 0; j0 -= 8) {
            double g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 - u >= 0 ? j0 - u : 0;
                g[u] = fabs(fma(-ts->de[j + 1].y, Ac[(j + 1) * ld], Xc[j * ld]));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 - u >= 0 && g[u] <= gbest) { gbest = g[u]; kk = j0 - u; }   // ties: the smallest index, in both waves alike
        }
    }
    __syncthreads();   // both waves have read every q before the z overwrite them
    if (wave == 0 && lane < na) {
        double z = 1.0, nrm2 = 1.0;
        for (int j0 = n - 2; j0 >= 0; j0 -= 8) {
            double f[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 - u >= 0 ? j0 - u : 0;
                double qq = Xc[j * ld];
                if (fabs(qq) < tiny) qq = -tiny;
                f[u] = -(ts->e[j] * nr_rcp(qq));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (j0 - u >= 0 && j0 - u < kk) {
                    z = f[u] * z;
                    Xc[(j0 - u) * ld] = z;
                    nrm2 = fma(z, z, nrm2);
                }
            }
        }
        Xc[kk * ld] = 1.0;
        ts->praw[lane] = nrm2;
    } else if (wave == 1 && lane < na) {
        double z = 1.0, nrm2 = 0.0;
        for (int j0 = 0; j0 + 1 < n; j0 += 8) {
            double f[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u + 1 < n ? j0 + u : 0;
                f[u] = -(ts->e[j] * Ac[(j + 1) * ld]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (j0 + u + 1 < n && j0 + u >= kk) {
                    z = f[u] * z;
                    Xc[(j0 + u + 1) * ld] = z;
                    nrm2 = fma(z, z, nrm2);
                }
            }
        }
        ts->uq[lane] = nrm2;
    }
    __syncthreads();
    if (tid < na) {
        const double nrm2 = ts->praw[tid] + ts->uq[tid];
        const bool ok = nrm2 > 0.0 && nrm2 < 1e300;
        ts->inv[tid] = nr_rsqrt(ok ? nrm2 : 1.0);
        if (!ok) ts->bad = 1;
    }
    __syncthreads();
    TSTAMP(5);
    // ---- residuals |T x - lambda x|_inf of the normalised vectors and orthogonality of X (clustered / repeated
    // eigenvalues), every thread / wave its share; then (4) Z = Q X into A
    {
        double worst = 0.0;
        bool bad = false;
        for (int e0 = tid; e0 < n * na; e0 += nt) {
            const int j = e0 / na, i = e0 - j * na;
            const double x0 = X[j * ld + i];
            const double xm = j > 0 ? ts->e[j - 1] * X[(j - 1) * ld + i] : 0.0;
            const double xp = j + 1 < n ? ts->e[j] * X[(j + 1) * ld + i] : 0.0;
            const double tx = fma(ts->d[j] - ts->lam[i], x0, xm + xp) * ts->inv[i];
            bad = bad || !(fabs(tx) <= 1e-10);   // scaled matrix: |T| <= 1
        }
        const int jj = lane & 15, g = lane >> 4;
        const int tiles = (na + 15) >> 4;
        for (int t = wave; t < tiles * tiles; t += nt >> 6) {
            const int a0 = (t / tiles) * 16, b0 = (t - (t / tiles) * tiles) * 16;
            if (b0 > a0) continue;   // X'X is symmetric
            const bool aok = a0 + jj < na, bok = b0 + jj < na;
            const int ai = aok ? a0 + jj : 0, bi = bok ? b0 + jj : 0;
            const double sa = ts->inv[ai], sb = ts->inv[bi];
            const v4f64 acc = mfma_tile_acc(
                n, g, aok, bok, [&](int k) { return X[k * ld + ai] * sa; }, [&](int k) { return X[k * ld + bi] * sb; });
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = a0 + g + 4 * r, col = b0 + jj;
                if (row < na && col < na) worst = fmax(worst, fabs(acc[r] - (row == col ? 1.0 : 0.0)));
            }
        }
        if (bad) worst = 1e300;
#pragma unroll   // written out like `an` in the bracket set-up above: see the comment there
        for (int off = 32; off > 0; off >>= 1) worst = fmax(worst, __shfl_xor(worst, off, 64));
        if (lane == 0) ts->red[wave] = worst;
        __syncthreads();
        worst = 0.0;
        for (int w = 0; w < nt / 64; ++w) worst = fmax(worst, ts->red[w]);
        TSTAMP(6);
        if (ts->bad || !(worst <= orth_tol)) return false;
    }
    mfma_mm<true, false>(A, Q, X, n, na, n, ld, ts->inv);   // Q holds Q'
    if (tid < na) ts->lam[tid] /= ts->scale;
    __syncthreads();
    TSTAMP(7);
    kept = na < n ? na : 0;
    return true;
}

// Eigenpairs of the symmetric n x n matrix in A (destroyed): tridiag_eigh when `try_tri` (A, V, X then sit in the LDS
// with stride kTriLd; X is not touched otherwise), and on its refusal Jacobi on the copy saved in `backup` (n * n,
// packed, global).  Eigenvalues to ev_out in solver order, vec = the matrix whose columns hold the eigenvectors
// (A after tridiag_eigh, V after Jacobi).  Returns the Jacobi sweeps, 0 for the tridiagonal path (tell the two apart
// by vec: Jacobi on a diagonal matrix takes 0 sweeps as well).  The caller synchronises before ev_out is read.
// want > 0: only the `want` pairs of largest |eigenvalue| will be read.  kept > 0 on return says that only `kept` pairs
// were computed (tridiag_eigh): ev_out[0 .. kept) and columns 0 .. kept - 1 of vec, in solver order; the `want` leading
// ones are among them and rank among them as among all n.  kept = 0: all n.
// Force-inlined: A, V, X must stay known LDS or known global pointers (see tica_solve_kernel).
__device__ __forceinline__ int eigh_with_fallback(double* A, double* V, double* X, int n, int ld, double* backup,
                                                  bool try_tri, TriShared* ts, JacobiShared* sh, double orth_tol,
                                                  double* ev_out, const double*& vec, int want, int& kept) {
    const int tid = threadIdx.x, nt = blockDim.x;
    kept = 0;
    if (try_tri) {
        for (int e = tid; e < n * n; e += nt) backup[e] = A[(e / n) * ld + (e % n)];
        __syncthreads();
        if (tridiag_eigh(A, V, X, n, ld, ts, orth_tol, want, sh->p, kept)) {
            for (int i = tid; i < (kept ? kept : n); i += nt) ev_out[i] = ts->lam[i];
            vec = A;
            return 0;
        }
        kept = 0;
        __syncthreads();
        for (int e = tid; e < n * n; e += nt) A[(e / n) * ld + (e % n)] = backup[e];
        __syncthreads();
    }
    const int sweeps = jacobi_eigh(A, V, n, ld, sh, 40);
    for (int i = tid; i < n; i += nt) ev_out[i] = A[i * ld + i];
    vec = V;
    return sweeps;
}

struct TicaWork {  // global scratch: four n*ld matrices, then ev[n], mean[n], isc[n], order[n]
    double *A, *V, *B1, *B2, *ev, *mean, *isc;
    int* order;
};

// moments = [M00 F*F][M0t F*F][sx F][sy F][T]   (centred by shift, unscaled)
// scale   = per-feature divisor applied to the centred data (NULL -> 1)
// lds_mats: how many of {A, V, B1, B2} live in LDS (4, 2 or 0)
// (template, not a runtime flag: a pointer that may be LDS or global forces slow FLAT accesses)
template <int lds_mats>
__global__ __launch_bounds__(kEigThreads) void tica_solve_kernel(
    const double* __restrict__ mom, const double* __restrict__ scale, int n, int ld, double epsilon, int kinetic_map,
    int n_lead, TicaWork wk, double* __restrict__ out_eig, double* __restrict__ out_W, double* __restrict__ out_mean,
    int* __restrict__ out_rank) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ JacobiShared sh;
    __shared__ TriShared ts;
    const int tid = threadIdx.x, nt = blockDim.x;
    double* lds = reinterpret_cast<double*>(smem_raw);
    const size_t mat = (size_t)n * ld;
    double *A, *V, *B1, *B2;
    if constexpr (lds_mats >= 2) { A = lds; V = lds + mat; } else { A = wk.A; V = wk.V; }
    if constexpr (lds_mats >= 4) { B1 = lds + 2 * mat; B2 = lds + 3 * mat; } else { B1 = wk.B1; B2 = wk.B2; }

    const double* M00 = mom;
    const double* M0t = mom + (size_t)n * n;
    const double* sx = M0t + (size_t)n * n;
    const double* sy = sx + n;
    const double T = sy[n];
    const double w = 2.0 * T;
    KSTAMP_INIT
    if (!(T > 0.0)) {
        if (tid == 0) *out_rank = 0;
        for (int i = tid; i < n; i += nt) { out_eig[i] = 0.0; out_mean[i] = 0.0; }
        for (int i = tid; i < n * n; i += nt) out_W[i] = 0.0;
        return;
    }
    // 1 / scale and the means: in the LDS when they fit the solver's arrays (they are read 2 n times each below)
    double* iscp = (lds_mats == 4 && n <= kTriMax) ? ts.lam : wk.isc;
    double* meanp = (lds_mats == 4 && n <= kTriMax) ? ts.inv : wk.mean;
    for (int i = tid; i < n; i += nt) {
        const double is = scale ? 1.0 / scale[i] : 1.0;
        iscp[i] = is;
        const double m = (sx[i] + sy[i]) / w * is;
        meanp[i] = m;
        out_mean[i] = m;
    }
    __syncthreads();
    auto build_cov = [&]() {
        for (int e = tid; e < n * n; e += nt) {
            const int i = e / n, j = e - i * n;
            const double ss = iscp[i] * iscp[j];
            const double mm = meanp[i] * meanp[j];
            A[i * ld + j] = 0.5 * (M00[e] + M00[j * n + i]) / w * ss - mm;   // C00
            B1[i * ld + j] = (M0t[e] + M0t[j * n + i]) / w * ss - mm;        // C0t
        }
        __syncthreads();
    };
    build_cov();
    KSTAMP(8);

    // ---- whitening L with L' C00 L = I -------------------------------------------------
    // deeptime's spd_inv_split keeps the eigen-directions of C00 with |s| >= epsilon.  When
    // ALL of them qualify (C00 - epsilon I positive definite: tested by a factorisation attempt)
    // the TICA eigenpairs do not depend on which whitening is used -- they solve
    // C0t r = lambda C00 r -- so L = chol(C00)^-T replaces the first eigensolve.
    // Rank-deficient C00 takes the eigen path below, as before.
    constexpr bool kFused = lds_mats == 4;   // fused LDL' + inverse (one barrier per four columns) and the tridiagonal solver
    bool full_rank;
    if (kFused && n <= kTriMax) {
        // B2 = whitening W (upper triangular, W' C00 W = I); C00 stays in A.  C00^-1 = W W', so lambda_min(C00) >=
        // 1 / trace(W W') = 1 / ||W||_F^2: when that already clears epsilon every eigen-direction is kept and the
        // elimination of the probe C00 - epsilon I (a second pass of the same length) is not needed
        full_rank = ldl_whiten_registers(A, B2, n, epsilon, &ts, 1);
        if (full_rank) {
            double s = 0.0;
            for (int e = tid; e < n * n; e += nt) {
                const double wv = B2[(e / n) * ld + (e % n)];
                s = fma(wv, wv, s);
            }
            s = block_sum_bcast(s, sh.red, sh.bc);
            if (!(s * epsilon * (1.0 + 1e-9) <= 1.0)) full_rank = ldl_whiten_registers(A, nullptr, n, epsilon, &ts, 2);
        }
    } else {
        for (int e = tid; e < n * n; e += nt) {
            const int i = e / n, j = e - i * n;
            B2[i * ld + j] = A[i * ld + j] - (i == j ? epsilon : 0.0);
            V[i * ld + j] = A[i * ld + j];
        }
        __syncthreads();
        full_rank = cholesky_lower_pair(B2, V, n, ld, &sh);   // probe on C00 - eps I, factor C00 = G G'
        if (full_rank) {
            lower_inverse(V, A, n, ld);         // A = G^-1 (lower)
            for (int e = tid; e < n * n; e += nt) {
                const int i = e / n, j = e - i * n;
                B2[i * ld + j] = j >= i ? A[j * ld + i] : 0.0;  // L = G^-T (upper)
            }
            __syncthreads();
        } else {
            __syncthreads();
            build_cov();
        }
    }
    KSTAMP(9);
    int rank;
    if (full_rank) {
        rank = n;
        if (tid == 0) *out_rank = n;
    } else {
        // ---- spd_inv_split(C00): eigh, sort by |ev| desc, cut at epsilon, canonical signs ----
        jacobi_eigh(A, V, n, ld, &sh, 40);
        for (int i = tid; i < n; i += nt) wk.ev[i] = A[i * ld + i];
        __syncthreads();
        sort_desc_abs(wk.ev, n, wk.order);
        if (tid == 0) {
            double evmin = wk.ev[0];
            for (int i = 1; i < n; ++i) evmin = fmin(evmin, wk.ev[i]);
            double eps = epsilon;
            if (evmin < 0.0) eps = fmax(eps, -evmin + 1e-16);
            int rank = 0;
            for (int i = 0; i < n; ++i) rank += fabs(wk.ev[i]) >= eps;
            sh.ibc[0] = rank;
            *out_rank = rank;
        }
        __syncthreads();
        rank = sh.ibc[0];
        if (rank == 0) {
            for (int i = tid; i < n; i += nt) out_eig[i] = 0.0;
            for (int i = tid; i < n * n; i += nt) out_W[i] = 0.0;
            return;
        }
        // L (in B2) = V[:, order[:rank]] with canonical signs, columns scaled by 1/sqrt(s)
        for (int e = tid; e < n * rank; e += nt) {
            const int i = e / rank, j = e - i * rank;
            B2[i * ld + j] = V[i * ld + wk.order[j]];
        }
        __syncthreads();
        canonical_signs(B2, n, rank, ld);
        for (int e = tid; e < n * rank; e += nt) {
            const int i = e / rank, j = e - i * rank;
            B2[i * ld + j] /= sqrt(wk.ev[wk.order[j]]);
        }
        __syncthreads();
    }
    // ---- Ct = L' C0t L: A <- C0t L, V <- L' A, A <- sym(V) ----
    mfma_mm<false, false>(A, B1, B2, n, rank, n, ld);
    mfma_mm<true, false>(V, B2, A, rank, rank, n, ld);
    for (int e = tid; e < rank * rank; e += nt) {
        const int i = e / rank, j = e - i * rank;
        A[i * ld + j] = 0.5 * (V[i * ld + j] + V[j * ld + i]);
    }
    __syncthreads();
    KSTAMP(10);
    // eigenpairs of the whitened C0t: tridiagonal solver (fallback: Jacobi on the saved copy)
    // only the first `keep` pairs (by |ev|) go out.  Where the LDS tail follows (F <= kTriMax, full rank or not) the
    // tridiagonal solver may compute just `kept` candidates for them, which that tail knows how to rank; the generic
    // tail (F = 65 with rank <= 64 reaches the tridiagonal solver too) and every other solver get all `rank` pairs,
    // kept = 0, and the tails truncate
    const int keep = n_lead > 0 && n_lead < rank ? n_lead : rank;
    const bool lds_tail = kFused && n <= kTriMax;
    const double* Vec;
    int kept;
    eigh_with_fallback(A, V, B1, rank, ld, wk.A, kFused && rank <= kTriMax, &ts, &sh, 1e-11, wk.ev, Vec,
                       lds_tail && keep < rank ? keep : 0, kept);
    __syncthreads();
    KSTAMP(11);
    if (lds_tail) {
        // ---- the same tail with everything small in the LDS: eigenvalues, their order (|ev| descending, stable), the
        // sign of every column of R = L Rt (its largest-magnitude entry, first occurrence, made positive); the signs
        // and the kinetic-map factors are applied on the way out instead of in place
        double* evl = ts.praw;      // eigenvalues in solver order
        double* sgn = ts.uq;        // +-1 per solver column
        int* ord = sh.p;            // ord[j] = solver column of the j-th largest |ev|
        const int ncol = kept ? kept : rank;   // solver columns at hand
        if (tid < ncol) evl[tid] = wk.ev[tid];
        __syncthreads();
        rank_order<true>(ncol, ord, [&](int i) { return fabs(evl[i]); });
        mfma_mm<false, false>(B1, B2, Vec, n, ncol, rank, ld);   // columns still in solver order (barrier inside)
        {
            const int lane = tid & 63, wave = tid >> 6;
            for (int j = wave; j < ncol; j += nt >> 6) {          // one wave per column, lane = row
                double best = lane < n ? fabs(B1[lane * ld + j]) : -1.0;
                int bi = lane;
                double val = lane < n ? B1[lane * ld + j] : 0.0;
                wave_argmax_xor(best, bi, val);
                if (lane == 0) sgn[j] = val < 0.0 ? -1.0 : 1.0;
            }
        }
        __syncthreads();
        for (int e = tid; e < n * n; e += nt) {
            const int i = e / n, j = e - i * n;
            double v = 0.0;
            if (j < keep) {
                const int c = ord[j];
                v = B1[i * ld + c] * sgn[c];
                if (kinetic_map) v *= evl[c];
            }
            out_W[e] = v;
        }
        for (int j = tid; j < n; j += nt) out_eig[j] = j < keep ? evl[ord[j]] : 0.0;
        KSTAMP(12);
        return;
    }
    sort_desc_abs(wk.ev, rank, wk.order);
    // ---- R = L Rt (sorted), canonical signs, kinetic map ----
    mfma_mm<false, false>(B1, B2, Vec, n, rank, rank, ld);   // columns still in solver order
    canonical_signs(B1, n, rank, ld);
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, j = e - i * n;
        double v = 0.0;
        if (j < keep) {
            v = B1[i * ld + wk.order[j]];
            if (kinetic_map) v *= wk.ev[wk.order[j]];
        }
        out_W[e] = v;
    }
    for (int j = tid; j < n; j += nt) out_eig[j] = j < keep ? wk.ev[wk.order[j]] : 0.0;
    KSTAMP(12);
}

// Plain symmetric eigendecomposition (ascending eigenvalues), for tests and the
// reversible MSM path.
template <bool use_lds>
__global__ __launch_bounds__(kEigThreads) void eigh_kernel(const double* __restrict__ Ain, int n, int ld,
                                                          double* gA, double* gV, int* order,
                                                          double* __restrict__ out_w, double* __restrict__ out_v,
                                                          int* __restrict__ out_sweeps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ JacobiShared sh;
    __shared__ TriShared ts;   // only eigh_kernel<true> touches it
    const int tid = threadIdx.x, nt = blockDim.x;
    double *A, *V;
    if constexpr (use_lds) { A = reinterpret_cast<double*>(smem_raw); V = A + (size_t)n * ld; }
    else { A = gA; V = gV; }
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, j = e - i * n;
        A[i * ld + j] = 0.5 * (Ain[e] + Ain[j * n + i]);
    }
    __syncthreads();
    // up to kTriMax three LDS matrices were requested (jacobi_lds_bytes): the third is the tridiagonal solver's X.
    // out_w takes the eigenvalues in solver order first: final on the tridiagonal path, which yields them ascending
    const double* vec;
    int kept;   // all pairs are asked for: stays 0
    const int sweeps = eigh_with_fallback(A, V, V + (size_t)n * ld, n, ld, gA, use_lds && n <= kTriMax, &ts, &sh, 1e-12,
                                          out_w, vec, 0, kept);
    if (vec == A) {
        if (out_v)
            for (int e = tid; e < n * n; e += nt) out_v[e] = A[(e / n) * ld + (e % n)];
        if (tid == 0 && out_sweeps) *out_sweeps = 0;
        return;
    }
    // Jacobi: ascending order by value
    rank_order<false>(n, order, [&](int i) { return A[i * ld + i]; });
    __syncthreads();
    for (int j = tid; j < n; j += nt) out_w[j] = A[order[j] * ld + order[j]];
    if (out_v)
        for (int e = tid; e < n * n; e += nt) {
            const int i = e / n, j = e - i * n;
            out_v[e] = V[i * ld + order[j]];
        }
    if (tid == 0 && out_sweeps) *out_sweeps = sweeps;
}

// Eigenvalue estimator of the reference's DeepTICA trainer (_estimate_top_eigenvalues,
// S/features/deeptica/core/trainer_api.py:632-656) from ONE-SIDED raw moments (msm_lagged_moments_onesided):
//   C0 = (M00 - sx sx'/T) / max(1, T-1),  Ct = (M0t - sx sy'/T) / max(1, T-1)      (separate means of y_t, y_tau)
//   eigh(sym C0), eigenvalues clipped at `clip`; S = V diag(w^-1/2) V';  eigvalsh(sym(S Ct S')), descending.
// Four n x n matrices P0..P3 (LDS when they fit, else global), eigensolves by tridiag_eigh with the Jacobi fallback.
template <bool use_lds>
__global__ __launch_bounds__(kEigThreads) void onesided_eig_kernel(const double* __restrict__ mom, int n, int ld,
                                                                  double clip, double* gP, double* gbak, double* gw,
                                                                  int* order, double* __restrict__ out_eig) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ JacobiShared sh;
    __shared__ TriShared ts;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t mat = (size_t)n * ld;
    double* P0 = use_lds ? reinterpret_cast<double*>(smem_raw) : gP;
    double *P1 = P0 + mat, *P2 = P0 + 2 * mat, *P3 = P0 + 3 * mat;
    const double* M00 = mom;
    const double* M0t = mom + (size_t)n * n;
    const double* sx = M0t + (size_t)n * n;
    const double* sy = sx + n;
    const double T = sy[n];
    if (!(T > 0.0)) {
        for (int i = tid; i < n; i += nt) out_eig[i] = 0.0;
        return;
    }
    const double den = T - 1.0 > 1.0 ? T - 1.0 : 1.0;
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, j = e - i * n;
        const double c0 = 0.5 * (M00[e] + M00[j * n + i]) - sx[i] * sx[j] / T;
        P0[i * ld + j] = c0 / den;
        P1[i * ld + j] = (M0t[e] - sx[i] * sy[j] / T) / den;
    }
    __syncthreads();
    // eigenpairs of the symmetric matrix in P0 (work P2, P3): eigenvalues to gw, eigenvectors to *vec
    auto eigh = [&](const double*& vec) {
        int kept;   // all pairs are asked for: stays 0
        eigh_with_fallback(P0, P2, P3, n, ld, gbak, use_lds && n <= kTriMax, &ts, &sh, 1e-12, gw, vec, 0, kept);
        __syncthreads();
    };
    const double* vec = nullptr;
    eigh(vec);
    // P3 = V diag(w^-1/4): S = P3 P3'
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, j = e - i * n;
        const double wj = gw[j] > clip ? gw[j] : clip;
        P3[i * ld + j] = vec[i * ld + j] / sqrt(sqrt(wj));
    }
    __syncthreads();
    mfma_mm<false, true>(P0, P3, P3, n, n, n, ld);   // S -> P0
    mfma_mm<false, false>(P2, P0, P1, n, n, n, ld);   // S Ct
    mfma_mm<false, false>(P3, P2, P0, n, n, n, ld);   // (S Ct) S'   (S is symmetric)
    for (int e = tid; e < n * n; e += nt) {
        const int i = e / n, j = e - i * n;
        P0[i * ld + j] = 0.5 * (P3[i * ld + j] + P3[j * ld + i]);
    }
    __syncthreads();
    eigh(vec);
    rank_order<true>(n, order, [&](int i) { return gw[i]; });   // descending
    __syncthreads();
    for (int j = tid; j < n; j += nt) out_eig[j] = gw[order[j]];
}

size_t jacobi_lds_bytes(int n, int ld) { return (size_t)(n <= kTriMax ? 3 : 2) * n * ld * sizeof(double); }

// A workgroup has 160 KiB of LDS on gfx950, and the kernels' own __shared__ structs come out of it: a dynamic request
// that does not leave room for them makes hipFuncSetAttribute fail.  Every kernel that can reach tridiag_eigh carries
// both structs; tica_solve_kernel<2> and <0> never touch the TriShared one.  tests/_eig_ref.py restates these sizes.
constexpr size_t kLdsPerWorkgroup = 160 * 1024;
constexpr size_t kStaticLdsJacobi = sizeof(JacobiShared);
constexpr size_t kStaticLdsTri = sizeof(JacobiShared) + sizeof(TriShared);
static_assert(sizeof(JacobiShared) == 5808 && sizeof(TriShared) == 21808, "update the sizes restated in tests/_eig_ref.py");
constexpr size_t lds_cap(size_t budget, size_t static_bytes) {
    return budget < kLdsPerWorkgroup - static_bytes ? budget : kLdsPerWorkgroup - static_bytes;
}

// odd row stride; the fixed one of the tridiagonal solver up to its largest order
int eig_ld(int n) { return n <= kTriMax ? kTriLd : (n | 1); }

// One workgroup of kEigThreads with `lds_bytes` of dynamic LDS on the context's stream.
template <typename... Params, typename... Args>
msm_status launch_single_workgroup(msm_ctx* ctx, void (*kern)(Params...), size_t lds_bytes, Args... args) {
    if (lds_bytes > 48 * 1024)
        MSM_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL(kern, dim3(1), dim3(kEigThreads), lds_bytes, ctx->stream, args...);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // namespace

#include "eig_large.h"   // orders 257 .. 2048: the device-wide block Jacobi and the solves built on it

extern "C" {

msm_status msm_tica_solve(msm_ctx* ctx, const double* d_moments, const double* d_scale, int F, double epsilon,
                          int kinetic_map, double* d_eigvals, double* d_coeffs, double* d_mean, int* d_rank) {
    return msm_tica_solve_leading(ctx, d_moments, d_scale, F, epsilon, kinetic_map, d_eigvals, d_coeffs, d_mean, d_rank, 0);
}

msm_status msm_tica_solve_leading(msm_ctx* ctx, const double* d_moments, const double* d_scale, int F, double epsilon,
                                  int kinetic_map, double* d_eigvals, double* d_coeffs, double* d_mean, int* d_rank,
                                  int n_lead) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, F >= 1, "msm_tica_solve: need F >= 1 (got %d)", F);
    if (F > kBjMaxOrder)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_tica_solve: F = %d exceeds the largest supported order %d", F, kBjMaxOrder);
    MSM_REQUIRE(ctx, epsilon >= 0.0, "msm_tica_solve: epsilon must be >= 0");
    MSM_REQUIRE(ctx, d_moments && d_eigvals && d_coeffs && d_mean && d_rank, "msm_tica_solve: NULL pointer");
    if (F > 2 * kMaxPairs)
        return bj_tica_solve(ctx, d_moments, d_scale, F, epsilon, kinetic_map, d_eigvals, d_coeffs, d_mean, d_rank,
                             n_lead > 0 && n_lead < F ? n_lead : 0);
    const int ld = eig_ld(F);
    const size_t mat = (size_t)F * ld;
    const size_t need = (4 * mat + 3 * F) * sizeof(double) + (size_t)F * sizeof(int) + 64;
    msm_status rs = msm_reserve_scratch(ctx, need);
    if (rs != MSM_OK) return rs;
    double* base = (double*)ctx->scratch;
    TicaWork wk;
    wk.A = base; wk.V = base + mat; wk.B1 = base + 2 * mat; wk.B2 = base + 3 * mat;
    wk.ev = base + 4 * mat; wk.mean = wk.ev + F; wk.isc = wk.mean + F; wk.order = (int*)(wk.isc + F);
    const size_t lds_budget = 150 * 1024;
    int lds_mats = 0;
    if (4 * mat * sizeof(double) <= lds_cap(lds_budget, kStaticLdsTri)) lds_mats = 4;
    else if (2 * mat * sizeof(double) <= lds_cap(lds_budget, kStaticLdsJacobi)) lds_mats = 2;
    const size_t lds = (size_t)lds_mats * mat * sizeof(double);
    auto kern = lds_mats == 4 ? tica_solve_kernel<4> : (lds_mats == 2 ? tica_solve_kernel<2> : tica_solve_kernel<0>);
    return launch_single_workgroup(ctx, kern, lds, d_moments, d_scale, F, ld, epsilon, kinetic_map,
                                   n_lead > 0 && n_lead < F ? n_lead : 0, wk, d_eigvals, d_coeffs, d_mean, d_rank);
}

msm_status msm_onesided_tica_eigenvalues(msm_ctx* ctx, const double* d_moments, int F, double clip, double* d_eigvals) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, F >= 1, "msm_onesided_tica_eigenvalues: need F >= 1 (got %d)", F);
    if (F > kBjMaxOrder)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_onesided_tica_eigenvalues: F = %d exceeds the largest supported order %d",
                        F, kBjMaxOrder);
    MSM_REQUIRE(ctx, d_moments && d_eigvals && clip > 0.0, "msm_onesided_tica_eigenvalues: bad arguments");
    if (F > 2 * kMaxPairs) return bj_onesided(ctx, d_moments, F, clip, d_eigvals);
    const int ld = eig_ld(F);
    const size_t mat = (size_t)F * ld;
    const size_t lds = 4 * mat * sizeof(double);
    const bool use_lds = lds <= lds_cap(140 * 1024, kStaticLdsTri);
    msm_status rs = msm_reserve_scratch(ctx, ((use_lds ? 0 : 4 * mat) + (size_t)F * F + F) * sizeof(double) +
                                                 (size_t)F * sizeof(int) + 64);
    if (rs != MSM_OK) return rs;
    double* gP = (double*)ctx->scratch;
    double* gbak = gP + (use_lds ? 0 : 4 * mat);
    double* gw = gbak + (size_t)F * F;
    int* order = (int*)(gw + F);
    auto kern = use_lds ? onesided_eig_kernel<true> : onesided_eig_kernel<false>;
    return launch_single_workgroup(ctx, kern, use_lds ? lds : 0, d_moments, F, ld, clip, gP, gbak, gw, order, d_eigvals);
}

msm_status msm_eigh(msm_ctx* ctx, const double* d_a, int n, double* d_w, double* d_v, int* d_sweeps) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n >= 1, "msm_eigh: need n >= 1 (got %d)", n);
    if (n > kBjMaxOrder)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_eigh: n = %d exceeds the largest supported order %d", n, kBjMaxOrder);
    MSM_REQUIRE(ctx, d_a && d_w, "msm_eigh: NULL pointer");
    if (n > 2 * kMaxPairs) return bj_eigh(ctx, d_a, n, d_w, d_v, d_sweeps);
    const int ld = eig_ld(n);
    const size_t mat = (size_t)n * ld;
    msm_status rs = msm_reserve_scratch(ctx, 2 * mat * sizeof(double) + (size_t)n * sizeof(int) + 64);
    if (rs != MSM_OK) return rs;
    double* gA = (double*)ctx->scratch;
    double* gV = gA + mat;
    int* order = (int*)(gV + mat);
    const size_t lds = jacobi_lds_bytes(n, ld);
    const int use_lds = lds <= lds_cap(140 * 1024, kStaticLdsTri);
    auto kern = use_lds ? eigh_kernel<true> : eigh_kernel<false>;
    return launch_single_workgroup(ctx, kern, use_lds ? lds : 0, d_a, n, ld, gA, gV, order, d_w, d_v, d_sweeps);
}

}  // extern "C"
