// Per-frame featurizers: pair distances, three-body angles, dihedrals (+ cos/sin).
//
// HBM-bound: read 12*A bytes of coordinates per frame, write 4 bytes per feature
// (SURVEY.md section 8d).  Threads are laid out feature-fastest so the output rows are
// written as contiguous runs; the (few hundred bytes of) coordinates of a frame are
// shared by all its features through L1.  Arithmetic is fp32 in the operation order
// of the reference's in-repo extractor (S/features/deeptica/ts_feature_extractor.py:
// 423-500): d = sqrt(max(|v|^2, eps)); angle = acos(clamp(v1.v2/(|v1||v2|)));
// dihedral = atan2((c0 x c1).b1/|b1|, c0.c1) with c0 = b0 x b1, c1 = b1 x b2 normalised.
// The per-kind kernels know no periodic box; spec_kernel takes a mixed feature list and
// replaces flagged bond vectors by their minimum image (pbc.h) before the same arithmetic.
#include <cfloat>

#include "common.h"
#include "pbc.h"
#include "wave.h"

namespace {

constexpr int kThreads = 256;

// the three geometries on bond vectors (pbc.h has V3 and kEps); every kernel below goes through these, so a
// minimum-image vector and a plain difference meet the same operations in the same order.  The floor and the clamp
// are comparisons, not fmaxf / fminf, which return the operand that is not NaN: a NaN coordinate stays NaN, as with
// torch.clamp_min / torch.clamp in the reference (finite input: the same bits either way).
__device__ __forceinline__ float floor_keep_nan(float q) { return q < kEps ? kEps : q; }
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float distance_of(V3 v) { return sqrtf(floor_keep_nan(dot(v, v))); }

__device__ __forceinline__ float angle_of(V3 v1, V3 v2) {
    const float n1 = sqrtf(floor_keep_nan(dot(v1, v1)));
    const float n2 = sqrtf(floor_keep_nan(dot(v2, v2)));
    const float c = dot(v1, v2) / (n1 * n2);
    return acosf(clamp_keep_nan(c, -1.0f, 1.0f));
}

__device__ __forceinline__ float dihedral_of(V3 b0, V3 b1, V3 b2) {
    V3 c0 = cross(b0, b1), c1 = cross(b1, b2);
    const float n0 = sqrtf(floor_keep_nan(dot(c0, c0)));
    const float n1 = sqrtf(floor_keep_nan(dot(c1, c1)));
    const float nb = sqrtf(floor_keep_nan(dot(b1, b1)));
    c0 = scale(c0, n0);
    c1 = scale(c1, n1);
    const V3 b1u = scale(b1, nb);
    const float x = dot(c0, c1);
    const float y = dot(cross(c0, c1), b1u);
    const bool ok = (fabsf(x) + fabsf(y)) >= kEps;
    float ang = ok ? atan2f(y, x) : 0.0f;
    if (ang <= -3.14159265358979323846f) ang += 6.28318530717958647692f;  // builtins.py:11-14
    return ang;
}

__global__ __launch_bounds__(kThreads) void distances_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                            const int* __restrict__ pairs, int P,
                                                            float* __restrict__ out, int64_t ld, int col_off) {
    const int64_t total = n * P;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t t = e / P;
        const int f = (int)(e - t * P);
        const float* fr = xyz + t * A * 3;
        const V3 v = sub(ld3(fr + 3 * pairs[2 * f + 1]), ld3(fr + 3 * pairs[2 * f]));
        out[t * ld + col_off + f] = distance_of(v);
    }
}

__global__ __launch_bounds__(kThreads) void angles_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                         const int* __restrict__ trip, int Tn,
                                                         float* __restrict__ out, int64_t ld, int col_off) {
    const int64_t total = n * Tn;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t t = e / Tn;
        const int f = (int)(e - t * Tn);
        const float* fr = xyz + t * A * 3;
        const V3 pj = ld3(fr + 3 * trip[3 * f + 1]);
        const V3 v1 = sub(ld3(fr + 3 * trip[3 * f]), pj);
        const V3 v2 = sub(ld3(fr + 3 * trip[3 * f + 2]), pj);
        out[t * ld + col_off + f] = angle_of(v1, v2);
    }
}

// mode 0: angle in (-pi, pi];  mode 1: [cos, sin] adjacent per angle (api/features.py:138-180);
// mode 2: [cos block | sin block] (markov_state_model/_features.py:131-142)
__global__ __launch_bounds__(kThreads) void dihedrals_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                            const int* __restrict__ quads, int Q, int mode,
                                                            float* __restrict__ out, int64_t ld, int col_off) {
    const int64_t total = n * Q;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t t = e / Q;
        const int f = (int)(e - t * Q);
        const float* fr = xyz + t * A * 3;
        const V3 p0 = ld3(fr + 3 * quads[4 * f]), p1 = ld3(fr + 3 * quads[4 * f + 1]);
        const V3 p2 = ld3(fr + 3 * quads[4 * f + 2]), p3 = ld3(fr + 3 * quads[4 * f + 3]);
        const V3 b0 = sub(p1, p0), b1 = sub(p2, p1), b2 = sub(p3, p2);
        const float ang = dihedral_of(b0, b1, b2);
        float* row = out + t * ld + col_off;
        if (mode == 0) row[f] = ang;
        else if (mode == 1) { row[2 * f] = cosf(ang); row[2 * f + 1] = sinf(ang); }
        else { row[f] = cosf(ang); row[Q + f] = sinf(ang); }
    }
}

// contact indicator of one atom pair per column: 1.0 when the distance is <= rcut, else 0.0; a NaN
// distance (missing coordinates; distance_of keeps the NaN) or an infinite one counts as "no contact"
// (S/features/builtins.py:252-275 sets NaN to inf before it compares)
__global__ __launch_bounds__(kThreads) void contacts_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                           const int* __restrict__ pairs, int P, float rcut,
                                                           float* __restrict__ out, int64_t ld, int col_off) {
    const int64_t total = n * P;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t t = e / P;
        const int f = (int)(e - t * P);
        const float* fr = xyz + t * A * 3;
        const V3 v = sub(ld3(fr + 3 * pairs[2 * f + 1]), ld3(fr + 3 * pairs[2 * f]));
        const float dist = distance_of(v);
        out[t * ld + col_off + f] = dist <= rcut ? 1.0f : 0.0f;   // NaN compares false
    }
}

// radius of gyration with unit masses (mdtraj.compute_rg as called at S/features/builtins.py:98):
// sqrt(mean_a |r_a - mean_a r_a|^2); one wave per frame, fp64 accumulation of the fp32 coordinates
__global__ __launch_bounds__(kThreads) void rg_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                     float* __restrict__ out, int64_t ld, int col_off) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kThreads) >> 6;
    for (int64_t t = wave; t < n; t += n_waves) {
        const float* fr = xyz + t * A * 3;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int a = lane; a < A; a += 64) { sx += fr[3 * a]; sy += fr[3 * a + 1]; sz += fr[3 * a + 2]; }
        sx = wave_sum_xor(sx);
        sy = wave_sum_xor(sy);
        sz = wave_sum_xor(sz);
        const double mx = sx / A, my = sy / A, mz = sz / A;
        double q = 0.0;
        for (int a = lane; a < A; a += 64) {
            const double dx = fr[3 * a] - mx, dy = fr[3 * a + 1] - my, dz = fr[3 * a + 2] - mz;
            q += dx * dx + dy * dy + dz * dz;
        }
        q = wave_sum_xor(q);
        if (lane == 0) out[t * ld + col_off] = (float)sqrt(q / A);
    }
}

// One launch for a mixed feature list (msmhip.h: msm_featurize_spec has the record layout).  A block works on tiles
// of `tile_frames` consecutive frames (about kTileElems elements, at most kTileFrames frames).  Inside a tile the
// elements are ordered kind by kind -- all distances of the tile's frames, then all angles, dihedrals, contacts --
// and feature-fastest inside a kind, so a wave meets one kind except where two kinds join, and a row's columns of a
// kind are still written as one contiguous run.  (Element order t F + f puts every kind into nearly every wave once
// F is below 64, and each wave then pays for the dihedral path.)  The kinds' record ranges are read off the table
// by the block itself; a table that is not sorted by kind is still computed correctly, only with divergent waves.
// With boxes, the block first turns the boxes of the tile's frames (the one box of n_box = 1 once, ahead of the
// loop) into box | inverse | search radius in LDS.  Every thread runs every trip, so the barriers are uniform.
constexpr int kTileElems = 1024;
constexpr int kTileFrames = 256;

// kNanIn (the bias potential's forward): a record that reads a non-finite coordinate writes NaN.  Without the flag
// (msm_featurize_spec) the geometry follows the reference's rules: a NaN coordinate gives a NaN distance or angle, but a
// dihedral of 0 (its mask) and a contact of 0, and a lone infinite coordinate gives a +inf distance.
__device__ __forceinline__ bool finite3(V3 v) { return fabsf(v.x) <= FLT_MAX && fabsf(v.y) <= FLT_MAX && fabsf(v.z) <= FLT_MAX; }

template <bool kSearch, bool kNanIn>
__global__ __launch_bounds__(kThreads, 6) void spec_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                       const float* __restrict__ box, int64_t n_box,
                                                       const int4* __restrict__ rec, const float* __restrict__ param,
                                                       int F, int width, int tile_frames, float* __restrict__ out,
                                                       int64_t ld, int col_off) {
    __shared__ float s_box[kTileFrames * kBoxWords];
    __shared__ int s_bound[4];   // first record of kind >= k (k = 1, 2, 3)
    const bool per_frame = box != nullptr && n_box != 1;
    if (threadIdx.x < 4) s_bound[threadIdx.x] = F;
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += kThreads) {
        const int k = min(max(rec[2 * f].x, 0), 3), before = f ? min(max(rec[2 * f - 2].x, 0), 3) : 0;
        for (int kk = before + 1; kk <= k; ++kk) atomicMin(&s_bound[kk], f);
    }
    if (box != nullptr && !per_frame && threadIdx.x == 0) box_inverse(box, s_box);
    __syncthreads();
    const int b1 = s_bound[1], b2 = max(b1, s_bound[2]), b3 = max(b2, s_bound[3]);
    const int c0 = b1, c1 = b2 - b1, c2 = b3 - b2, c3 = F - b3;
    for (int64_t t0 = (int64_t)blockIdx.x * tile_frames; t0 < n; t0 += (int64_t)gridDim.x * tile_frames) {
        const int nf = (int)min((int64_t)tile_frames, n - t0);
        if (per_frame) {
            __syncthreads();   // the previous trip's readers are done
            for (int i = threadIdx.x; i < nf; i += kThreads) box_inverse(box + (t0 + i) * 9, s_box + i * kBoxWords);
            __syncthreads();
        }
        const int e0 = nf * c0, e1 = e0 + nf * c1, e2 = e1 + nf * c2;
        for (int j = threadIdx.x; j < nf * F; j += kThreads) {
            int r = j, first = 0, count = c0;
            if (j >= e2) { r = j - e2; first = b3; count = c3; }
            else if (j >= e1) { r = j - e1; first = b2; count = c2; }
            else if (j >= e0) { r = j - e0; first = b1; count = c1; }
            const int tl = r / count;
            const int f = first + (r - tl * count);
            const int64_t t = t0 + tl;
            const int4 r0 = rec[2 * f], r1 = rec[2 * f + 1];
            const int kind = r0.x, i0 = r0.y, i1 = r0.z, i2 = r0.w, i3 = r1.x, flags = r1.y, col = r1.z, col2 = r1.w;
            const float par = param[f];
            const bool trig = kind == MSM_FEAT_DIHEDRAL && (flags & MSM_FEAT_COSSIN);
            if (col < 0 || col >= width || (trig && (col2 < 0 || col2 >= width))) continue;   // never outside the block
            const int n_atoms = kind == MSM_FEAT_DIHEDRAL ? 4 : (kind == MSM_FEAT_ANGLE ? 3 : 2);
            bool valid = (unsigned)kind <= (unsigned)MSM_FEAT_CONTACT && (unsigned)i0 < (unsigned)A && (unsigned)i1 < (unsigned)A;
            valid = valid && (n_atoms < 3 || (unsigned)i2 < (unsigned)A) && (n_atoms < 4 || (unsigned)i3 < (unsigned)A);
            const bool wrap = box != nullptr && (flags & MSM_FEAT_MIC);
            const float* w = s_box + (per_frame ? tl * kBoxWords : 0);
            if (wrap && w[18] < 0.0f) valid = false;
            float* row = out + t * ld + col_off;
            const float* fr = xyz + t * A * 3;
            if (kNanIn && valid)
                valid = finite3(ld3(fr + 3 * i0)) && finite3(ld3(fr + 3 * i1)) && (n_atoms < 3 || finite3(ld3(fr + 3 * i2))) &&
                        (n_atoms < 4 || finite3(ld3(fr + 3 * i3)));
            if (!valid) {
                row[col] = __builtin_nanf("");
                if (trig) row[col2] = __builtin_nanf("");
                continue;
            }
            if (kind == MSM_FEAT_DISTANCE || kind == MSM_FEAT_CONTACT) {
                V3 v = sub(ld3(fr + 3 * i1), ld3(fr + 3 * i0));
                if (wrap) v = minimum_image<kSearch>(v, w);
                const float d = distance_of(v);
                row[col] = kind == MSM_FEAT_DISTANCE ? d * par : (d <= par ? 1.0f : 0.0f);
            } else if (kind == MSM_FEAT_ANGLE) {
                const V3 pj = ld3(fr + 3 * i1);
                V3 v1 = sub(ld3(fr + 3 * i0), pj);
                V3 v2 = sub(ld3(fr + 3 * i2), pj);
                if (wrap) { v1 = minimum_image<kSearch>(v1, w); v2 = minimum_image<kSearch>(v2, w); }
                row[col] = angle_of(v1, v2) * par;
            } else {
                const V3 p0 = ld3(fr + 3 * i0), p1 = ld3(fr + 3 * i1), p2 = ld3(fr + 3 * i2), p3 = ld3(fr + 3 * i3);
                V3 b0 = sub(p1, p0), b1v = sub(p2, p1), b2v = sub(p3, p2);
                if (wrap) {
                    b0 = minimum_image<kSearch>(b0, w);
                    b1v = minimum_image<kSearch>(b1v, w);
                    b2v = minimum_image<kSearch>(b2v, w);
                }
                const float ang = dihedral_of(b0, b1v, b2v);
                if (trig) { row[col] = cosf(ang) * par; row[col2] = sinf(ang) * par; }
                else row[col] = ang * par;
            }
        }
    }
}

// ---- the adjoint of spec_kernel (msmhip.h: msm_featurize_spec_vjp) ----------------------------------------------
// Bond vectors are the forward's (fp32 difference, the same minimum_image call), widened to fp64; the image shift is
// piecewise constant, so they differentiate like plain differences.  Everything below is fp64, written in the
// operation order of the restatement the tests hold it to.
struct D3 { double x, y, z; };
__device__ __forceinline__ D3 wide(V3 v) { return {(double)v.x, (double)v.y, (double)v.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ D3 over(D3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ D3 times(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ D3 plus(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 minus(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 neg(D3 a) { return {-a.x, -a.y, -a.z}; }

// What record (r0, r1) adds to atom a, which sits in its slot `slot`: upstream gradient times weight times the
// closed-form Jacobian of the slot.  Exactly zero for a contact, an unknown kind, a column outside the block, an atom
// outside [0, A), a slot that is not atom a's, a singular box under a flagged record, and wherever the forward's
// floor, clamp or mask is active (the conditions are written so that a NaN coordinate is not "degenerate": it
// propagates).  fr: the frame's coordinates; w: the frame's box words or nullptr; grow: the frame's gradient block.
template <bool kSearch>
__device__ __forceinline__ D3 vjp_entry(const float* __restrict__ fr, int A, const float* w, int4 r0, int4 r1,
                                        float par, int slot, int a, int width, const double* __restrict__ grow) {
    const D3 zero = {0.0, 0.0, 0.0};
    const int kind = r0.x, i0 = r0.y, i1 = r0.z, i2 = r0.w, i3 = r1.x, flags = r1.y, col = r1.z, col2 = r1.w;
    if ((unsigned)kind > (unsigned)MSM_FEAT_DIHEDRAL) return zero;
    const int n_atoms = kind == MSM_FEAT_DIHEDRAL ? 4 : (kind == MSM_FEAT_ANGLE ? 3 : 2);
    const bool trig = kind == MSM_FEAT_DIHEDRAL && (flags & MSM_FEAT_COSSIN);
    if (slot >= n_atoms || col < 0 || col >= width || (trig && (col2 < 0 || col2 >= width))) return zero;
    bool valid = (unsigned)i0 < (unsigned)A && (unsigned)i1 < (unsigned)A;
    valid = valid && (n_atoms < 3 || (unsigned)i2 < (unsigned)A) && (n_atoms < 4 || (unsigned)i3 < (unsigned)A);
    const int mine = slot == 0 ? i0 : (slot == 1 ? i1 : (slot == 2 ? i2 : i3));
    const bool wrap = w != nullptr && (flags & MSM_FEAT_MIC);
    if (!valid || mine != a || (wrap && w[18] < 0.0f)) return zero;
    const double eps = (double)kEps;
    if (kind == MSM_FEAT_DISTANCE) {
        V3 v = sub(ld3(fr + 3 * i1), ld3(fr + 3 * i0));
        if (wrap) v = minimum_image<kSearch>(v, w);
        const D3 d = wide(v);
        const double q = dot(d, d);
        if (q <= eps) return zero;
        const D3 j = over(d, sqrt(q));
        return times(grow[col] * (double)par, slot == 1 ? j : neg(j));
    }
    if (kind == MSM_FEAT_ANGLE) {
        const V3 pj = ld3(fr + 3 * i1);
        V3 f1 = sub(ld3(fr + 3 * i0), pj), f2 = sub(ld3(fr + 3 * i2), pj);
        if (wrap) { f1 = minimum_image<kSearch>(f1, w); f2 = minimum_image<kSearch>(f2, w); }
        const D3 v1 = wide(f1), v2 = wide(f2);
        const double q1 = dot(v1, v1), q2 = dot(v2, v2);
        const D3 nrm = cross(v1, v2);
        const double ww = dot(nrm, nrm);
        const double c = dot(v1, v2) / (sqrt(fmax(q1, eps)) * sqrt(fmax(q2, eps)));
        if (q1 <= eps || q2 <= eps || fabs(c) >= 1.0 || ww <= 0.0) return zero;
        const double nw = sqrt(ww);
        // d theta / d v1 = v1 x (v1 x v2) / (|v1|^2 |v1 x v2|), d theta / d v2 = -v2 x (v1 x v2) / (|v2|^2 |v1 x v2|):
        // -1 / sin(theta) d cos(theta) with the sine taken from the cross product, sound up to the collinear limit
        const D3 g1 = over(cross(v1, nrm), q1 * nw), g2 = neg(over(cross(v2, nrm), q2 * nw));
        const D3 j = slot == 0 ? g1 : (slot == 2 ? g2 : neg(plus(g1, g2)));
        return times(grow[col] * (double)par, j);
    }
    const V3 p0 = ld3(fr + 3 * i0), p1 = ld3(fr + 3 * i1), p2 = ld3(fr + 3 * i2), p3 = ld3(fr + 3 * i3);
    V3 e0 = sub(p1, p0), e1 = sub(p2, p1), e2 = sub(p3, p2);
    if (wrap) {
        e0 = minimum_image<kSearch>(e0, w);
        e1 = minimum_image<kSearch>(e1, w);
        e2 = minimum_image<kSearch>(e2, w);
    }
    const D3 b0 = wide(e0), b1 = wide(e1), b2 = wide(e2);
    const D3 c0 = cross(b0, b1), c1 = cross(b1, b2);
    const double q0 = dot(c0, c0), q1 = dot(c1, c1), qb = dot(b1, b1);
    if (q0 <= eps || q1 <= eps || qb <= eps) return zero;
    const double nb = sqrt(qb);
    const D3 u0 = over(c0, sqrt(q0)), u1 = over(c1, sqrt(q1));
    const double x = dot(u0, u1), y = dot(cross(u0, u1), over(b1, nb));
    if (fabs(x) + fabs(y) < eps) return zero;
    // the four-atom formula for phi = atan2(y, x) above: d phi / d x0 = -|b1| c0 / |c0|^2, d phi / d x3 = |b1| c1 / |c1|^2,
    // the inner atoms from them and the projections of b0, b2 on b1 (the four add up to zero)
    const D3 f1 = times(-(nb / q0), c0), f4 = times(nb / q1, c1);
    const double s01 = dot(b0, b1) / qb, s21 = dot(b2, b1) / qb;
    D3 j;
    if (slot == 0) j = f1;
    else if (slot == 3) j = f4;
    else if (slot == 1) j = plus(minus(neg(f1), times(s01, f1)), times(s21, f4));
    else j = minus(plus(neg(f4), times(s01, f1)), times(s21, f4));
    double coef = grow[col];
    if (trig) {   // cos(phi) = x / r, sin(phi) = y / r: no inverse trigonometry in the adjoint
        const double r = sqrt(x * x + y * y);
        coef = coef * -(y / r) + grow[col2] * (x / r);
    }
    return times(coef * (double)par, j);
}

// A block works on tiles of kVjpFrames consecutive frames; a thread owns one (frame, atom) of the tile and walks the
// atom's incidence entries in their (ascending) order, so the sum has one order whatever n is.  Threads are ordered
// frame-fastest inside an atom: with a full tile a wave is one atom's 64 frames, every lane walks the same entries and
// the wave never diverges; coordinates and gradients of a tile are a few KB that stay in L1.  Boxes as in spec_kernel.
// 3 A and nf * A fit an int: A <= 2^23 is checked by the entry point.
constexpr int kVjpFrames = 64;

template <bool kSearch>
__global__ __launch_bounds__(kThreads) void spec_vjp_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                           const float* __restrict__ box, int64_t n_box,
                                                           const int4* __restrict__ rec, const float* __restrict__ param,
                                                           int F, int width, const double* __restrict__ gfeat,
                                                           int64_t ldg, int col_off, const int* __restrict__ inc_ptr,
                                                           const int* __restrict__ inc, double sign,
                                                           double* __restrict__ gxyz) {
    __shared__ float s_box[kVjpFrames * kBoxWords];
    __shared__ int s_bad[kVjpFrames];   // the frame's gradient block holds a non-finite value
    const bool per_frame = box != nullptr && n_box != 1;
    if (box != nullptr && !per_frame && threadIdx.x == 0) box_inverse(box, s_box);
    for (int64_t t0 = (int64_t)blockIdx.x * kVjpFrames; t0 < n; t0 += (int64_t)gridDim.x * kVjpFrames) {
        const int nf = (int)min((int64_t)kVjpFrames, n - t0);
        __syncthreads();   // the previous trip's readers are done (first trip: the one box is in place after the next)
        for (int i = threadIdx.x; i < nf; i += kThreads) {
            if (per_frame) box_inverse(box + (t0 + i) * 9, s_box + i * kBoxWords);
            s_bad[i] = 0;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nf * width; e += kThreads) {
            const int tl = e / width;
            const double g = gfeat[(t0 + tl) * ldg + col_off + (e - tl * width)];
            if (!(fabs(g) <= DBL_MAX)) atomicOr(&s_bad[tl], 1);
        }
        __syncthreads();
        // atoms no record refers to (most atoms of a solvated system) get exact zeros, NaN in a poisoned frame, in one
        // coalesced sweep over the tile's contiguous block; the strided stores below are for referenced atoms only
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        double* tile = gxyz + t0 * A * 3;
        for (int tl = threadIdx.x >> 6; tl < nf; tl += kThreads / 64) {   // a wave per frame: its 3 A doubles are one run
            const double fill = s_bad[tl] ? qnan : 0.0;
            double* row = tile + (int64_t)tl * A * 3;
            for (int c = threadIdx.x & 63; c < 3 * A; c += 64) {
                const int a = c / 3;
                if (min(inc_ptr[a + 1], 4 * F) <= max(inc_ptr[a], 0)) row[c] = fill;
            }
        }
        for (int j = threadIdx.x; j < nf * A; j += kThreads) {
            const int a = j / nf, tl = j - a * nf;
            const int first = max(inc_ptr[a], 0), last = min(inc_ptr[a + 1], 4 * F);   // at most four slots a record
            if (first >= last) continue;
            const int64_t t = t0 + tl;
            const float* fr = xyz + t * A * 3;
            const float* w = box != nullptr ? s_box + (per_frame ? tl * kBoxWords : 0) : nullptr;
            const double* grow = gfeat + t * ldg + col_off;
            D3 acc = {0.0, 0.0, 0.0};
            for (int k = first; k < last; ++k) {
                const int code = inc[k], f = code >> 2;
                if (code < 0 || f >= F) continue;
                const D3 term = vjp_entry<kSearch>(fr, A, w, rec[2 * f], rec[2 * f + 1], param[f], code & 3, a, width, grow);
                acc = plus(acc, term);
            }
            double* out = tile + ((int64_t)tl * A + a) * 3;
            const bool bad = s_bad[tl] != 0;
            out[0] = bad ? qnan : sign * acc.x;
            out[1] = bad ? qnan : sign * acc.y;
            out[2] = bad ? qnan : sign * acc.z;
        }
    }
}

// cell [a, b, c (nm), alpha, beta, gamma (degrees)] -> box rows a, b, c with a along x and b in the xy-plane, as
// mdtraj's lengths_and_angles_to_box_vectors does it: fp64 throughout, components within 1e-6 of zero set to zero
// (cos 90 degrees is 6e-17 in fp64; an orthorhombic cell comes out exactly diagonal), one rounding to fp32
__global__ __launch_bounds__(kThreads) void box_from_cell_kernel(const double* __restrict__ cell, int64_t n,
                                                                float* __restrict__ box) {
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += (int64_t)gridDim.x * kThreads) {
        const double* c = cell + t * 6;
        const double rad = 3.14159265358979323846 / 180.0;
        const double ca = cos(c[3] * rad), cb = cos(c[4] * rad), cg = cos(c[5] * rad), sg = sin(c[5] * rad);
        double b[9] = {c[0], 0.0, 0.0, c[1] * cg, c[1] * sg, 0.0, 0.0, 0.0, 0.0};
        const double cx = c[2] * cb, cy = c[2] * (ca - cb * cg) / sg;
        b[6] = cx;
        b[7] = cy;
        b[8] = sqrt(c[2] * c[2] - cx * cx - cy * cy);
#pragma unroll
        for (int i = 0; i < 9; ++i) box[t * 9 + i] = (float)(fabs(b[i]) < 1.0e-6 ? 0.0 : b[i]);
    }
}

int grid_for(const msm_ctx* ctx, int64_t total) {
    return (int)std::min<int64_t>(std::max<int64_t>(1, (total + kThreads - 1) / kThreads), (int64_t)ctx->n_cu * 16);
}

msm_status check_common(msm_ctx* ctx, const char* who, const float* xyz, int64_t n, int A, const int32_t* idx, int m,
                        float* out, int64_t ld, int col_off, int width) {
    MSM_REQUIRE(ctx, n >= 0 && A >= 1 && m >= 0, "%s: need n >= 0, A >= 1, count >= 0", who);
    MSM_REQUIRE(ctx, col_off >= 0 && ld >= col_off + (int64_t)width, "%s: output columns [%d, %d) exceed ld=%lld", who,
                col_off, col_off + width, (long long)ld);
    MSM_REQUIRE(ctx, (n == 0 || m == 0) || (xyz && idx && out), "%s: NULL pointer", who);
    return MSM_OK;
}

}  // namespace

// msm_featurize_spec, and with nan_in the bias potential's forward (common.h)
msm_status featurize_spec_launch(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_box, int64_t n_box,
                                 const int32_t* d_rec, const float* d_param, int F, int width, int mic, float* d_out,
                                 int64_t ld, int col_off, bool nan_in) {
    if (!ctx) return MSM_ERR_INVALID;
    const char* who = "msm_featurize_spec";
    MSM_REQUIRE(ctx, n >= 0 && A >= 1 && F >= 0 && width >= 0, "%s: need n >= 0, A >= 1, F >= 0, width >= 0", who);
    MSM_REQUIRE(ctx, mic == MSM_MIC_ROUND || mic == MSM_MIC_SEARCH, "%s: mic must be MSM_MIC_ROUND or MSM_MIC_SEARCH, got %d",
                who, mic);
    MSM_REQUIRE(ctx, d_box ? (n_box == 1 || n_box == n) : n_box == 0,
                "%s: n_box=%lld must be 1 or n=%lld with a box, 0 without", who, (long long)n_box, (long long)n);
    MSM_REQUIRE(ctx, col_off >= 0 && ld >= col_off + (int64_t)width, "%s: output columns [%d, %d) exceed ld=%lld", who,
                col_off, col_off + width, (long long)ld);
    if (n == 0 || F == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_xyz && d_rec && d_param && d_out, "%s: NULL pointer", who);
    MSM_REQUIRE(ctx, ((uintptr_t)d_rec & 15) == 0, "%s: the record table must be 16-byte aligned", who);
    const int tile_frames = std::min(kTileFrames, std::max(1, kTileElems / F));
    const dim3 grid(grid_for(ctx, ((n + tile_frames - 1) / tile_frames) * kThreads)), block(kThreads);   // a block per tile, capped
    const int4* rec = reinterpret_cast<const int4*>(d_rec);
#define MSM_SPEC(S, N)                                                                                             \
    hipLaunchKernelGGL((spec_kernel<S, N>), grid, block, 0, ctx->stream, d_xyz, n, A, d_box, n_box, rec, d_param, F, \
                       width, tile_frames, d_out, ld, col_off)
    if (mic == MSM_MIC_SEARCH) {
        if (nan_in) MSM_SPEC(true, true);
        else MSM_SPEC(true, false);
    } else {
        if (nan_in) MSM_SPEC(false, true);
        else MSM_SPEC(false, false);
    }
#undef MSM_SPEC
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

extern "C" {

msm_status msm_featurize_distances(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_pairs, int P,
                                   float* d_out, int64_t ld, int col_off) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_common(ctx, "msm_featurize_distances", d_xyz, n, A, d_pairs, P, d_out, ld, col_off, P);
    if (rs != MSM_OK || n == 0 || P == 0) return rs;
    hipLaunchKernelGGL(distances_kernel, dim3(grid_for(ctx, n * P)), dim3(kThreads), 0, ctx->stream, d_xyz, n, A,
                       d_pairs, P, d_out, ld, col_off);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_featurize_contacts(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_pairs, int P,
                                  float rcut, float* d_out, int64_t ld, int col_off) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, rcut > 0.0f, "msm_featurize_contacts: rcut must be positive");
    msm_status rs = check_common(ctx, "msm_featurize_contacts", d_xyz, n, A, d_pairs, P, d_out, ld, col_off, P);
    if (rs != MSM_OK || n == 0 || P == 0) return rs;
    hipLaunchKernelGGL(contacts_kernel, dim3(grid_for(ctx, n * P)), dim3(kThreads), 0, ctx->stream, d_xyz, n, A, d_pairs,
                       P, rcut, d_out, ld, col_off);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_featurize_rg(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, float* d_out, int64_t ld, int col_off) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n >= 0 && A >= 1 && col_off >= 0 && ld >= col_off + 1, "msm_featurize_rg: bad shape");
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_xyz && d_out, "msm_featurize_rg: NULL pointer");
    hipLaunchKernelGGL(rg_kernel, dim3(grid_for(ctx, n * 64)), dim3(kThreads), 0, ctx->stream, d_xyz, n, A, d_out, ld,
                       col_off);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_featurize_angles(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_triplets, int Tn,
                                float* d_out, int64_t ld, int col_off) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_common(ctx, "msm_featurize_angles", d_xyz, n, A, d_triplets, Tn, d_out, ld, col_off, Tn);
    if (rs != MSM_OK || n == 0 || Tn == 0) return rs;
    hipLaunchKernelGGL(angles_kernel, dim3(grid_for(ctx, n * Tn)), dim3(kThreads), 0, ctx->stream, d_xyz, n, A,
                       d_triplets, Tn, d_out, ld, col_off);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_featurize_dihedrals(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_quads, int Q,
                                   int mode, float* d_out, int64_t ld, int col_off) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, mode >= 0 && mode <= 2, "msm_featurize_dihedrals: mode must be 0, 1 or 2");
    msm_status rs = check_common(ctx, "msm_featurize_dihedrals", d_xyz, n, A, d_quads, Q, d_out, ld, col_off,
                                 mode == 0 ? Q : 2 * Q);
    if (rs != MSM_OK || n == 0 || Q == 0) return rs;
    hipLaunchKernelGGL(dihedrals_kernel, dim3(grid_for(ctx, n * Q)), dim3(kThreads), 0, ctx->stream, d_xyz, n, A,
                       d_quads, Q, mode, d_out, ld, col_off);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_box_from_cell(msm_ctx* ctx, const double* d_cell, int64_t n, float* d_box) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n >= 0, "msm_box_from_cell: need n >= 0");
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_cell && d_box, "msm_box_from_cell: NULL pointer");
    hipLaunchKernelGGL(box_from_cell_kernel, dim3(grid_for(ctx, n)), dim3(kThreads), 0, ctx->stream, d_cell, n, d_box);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_featurize_spec(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_box, int64_t n_box,
                              const int32_t* d_rec, const float* d_param, int F, int width, int mic, float* d_out,
                              int64_t ld, int col_off) {
    return featurize_spec_launch(ctx, d_xyz, n, A, d_box, n_box, d_rec, d_param, F, width, mic, d_out, ld, col_off, false);
}

msm_status msm_featurize_spec_vjp(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_box, int64_t n_box,
                                  const int32_t* d_rec, const float* d_param, int F, int width, int mic,
                                  const double* d_gfeat, int64_t ldg, int col_off, const int32_t* d_inc_ptr,
                                  const int32_t* d_inc, double sign, double* d_gxyz) {
    if (!ctx) return MSM_ERR_INVALID;
    const char* who = "msm_featurize_spec_vjp";
    MSM_REQUIRE(ctx, n >= 0 && A >= 1 && F >= 0 && width >= 0, "%s: need n >= 0, A >= 1, F >= 0, width >= 0", who);
    MSM_REQUIRE(ctx, mic == MSM_MIC_ROUND || mic == MSM_MIC_SEARCH, "%s: mic must be MSM_MIC_ROUND or MSM_MIC_SEARCH, got %d",
                who, mic);
    MSM_REQUIRE(ctx, d_box ? (n_box == 1 || n_box == n) : n_box == 0,
                "%s: n_box=%lld must be 1 or n=%lld with a box, 0 without", who, (long long)n_box, (long long)n);
    MSM_REQUIRE(ctx, col_off >= 0 && ldg >= col_off + (int64_t)width, "%s: gradient columns [%d, %d) exceed ld=%lld", who,
                col_off, col_off + width, (long long)ldg);
    MSM_REQUIRE(ctx, F <= (1 << 28) && A <= (1 << 23), "%s: %d records, %d atoms (at most 2^28, 2^23)", who, F, A);
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_xyz && d_gxyz && d_inc_ptr && (width == 0 || d_gfeat), "%s: NULL pointer", who);
    MSM_REQUIRE(ctx, F == 0 || (d_rec && d_param && d_inc), "%s: NULL pointer", who);
    MSM_REQUIRE(ctx, ((uintptr_t)d_rec & 15) == 0, "%s: the record table must be 16-byte aligned", who);
    const dim3 grid(grid_for(ctx, ((n + kVjpFrames - 1) / kVjpFrames) * kThreads)), block(kThreads);   // a block per tile, capped
    const int4* rec = reinterpret_cast<const int4*>(d_rec);
    if (mic == MSM_MIC_SEARCH)
        hipLaunchKernelGGL(spec_vjp_kernel<true>, grid, block, 0, ctx->stream, d_xyz, n, A, d_box, n_box, rec, d_param, F,
                           width, d_gfeat, ldg, col_off, d_inc_ptr, d_inc, sign, d_gxyz);
    else
        hipLaunchKernelGGL(spec_vjp_kernel<false>, grid, block, 0, ctx->stream, d_xyz, n, A, d_box, n_box, rec, d_param, F,
                           width, d_gfeat, ldg, col_off, d_inc_ptr, d_inc, sign, d_gxyz);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
