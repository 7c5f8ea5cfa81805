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
#include "common.h"
#include "pbc.h"
#include "wave.h"

namespace {

constexpr int kThreads = 256;

// the three geometries on bond vectors (pbc.h has V3 and kEps); every kernel below goes through these, so a
// minimum-image vector and a plain difference meet the same operations in the same order
__device__ __forceinline__ float distance_of(V3 v) { return sqrtf(fmaxf(dot(v, v), kEps)); }

__device__ __forceinline__ float angle_of(V3 v1, V3 v2) {
    const float n1 = sqrtf(fmaxf(dot(v1, v1), kEps));
    const float n2 = sqrtf(fmaxf(dot(v2, v2), kEps));
    float c = dot(v1, v2) / (n1 * n2);
    c = fminf(fmaxf(c, -1.0f), 1.0f);
    return acosf(c);
}

__device__ __forceinline__ float dihedral_of(V3 b0, V3 b1, V3 b2) {
    V3 c0 = cross(b0, b1), c1 = cross(b1, b2);
    const float n0 = sqrtf(fmaxf(dot(c0, c0), kEps));
    const float n1 = sqrtf(fmaxf(dot(c1, c1), kEps));
    const float nb = sqrtf(fmaxf(dot(b1, b1), kEps));
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
// distance (missing coordinates) counts as "no contact" (S/features/builtins.py:252-275)
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

template <bool kSearch>
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
            if (!valid) {
                row[col] = __builtin_nanf("");
                if (trig) row[col2] = __builtin_nanf("");
                continue;
            }
            const float* fr = xyz + t * A * 3;
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
    if (mic == MSM_MIC_SEARCH)
        hipLaunchKernelGGL(spec_kernel<true>, grid, block, 0, ctx->stream, d_xyz, n, A, d_box, n_box, rec, d_param, F,
                           width, tile_frames, d_out, ld, col_off);
    else
        hipLaunchKernelGGL(spec_kernel<false>, grid, block, 0, ctx->stream, d_xyz, n, A, d_box, n_box, rec, d_param, F,
                           width, tile_frames, d_out, ld, col_off);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
