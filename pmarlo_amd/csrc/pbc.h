// Periodic boxes for the featurizers: the fp32 vector helpers every geometry kernel of featurize.hip works with,
// the closed-form inverse of a frame's box, and the two minimum-image rules.
//
// A box is 9 floats, rows a, b, c (mdtraj's unitcell_vectors: a along x, b in the xy-plane).  A bond vector v is a
// row vector, as in the reference's in-repo extractor (S/features/deeptica/ts_feature_extractor.py:414-421):
//   round : f = v . B^-1;  v' = (f - round(f)) . B            (round half to even, as torch.round)
//   search: additionally the 27 images v' + i a + j b + k c, i, j, k in {-1, 0, 1}, in the order
//           idx = 9 (i + 1) + 3 (j + 1) + (k + 1); the shortest wins, the lowest idx on a tie (mdtraj's rule for
//           triclinic cells; the true minimum image of any reduced cell).  Image 13 is v' itself, untouched, so the
//           two rules agree bit for bit wherever no other image is strictly shorter.  Every lattice vector other
//           than 0 is at least as long as the cell's smallest perpendicular width h (it crosses at least one pair
//           of opposite faces), so an image of v' other than v' is longer than h - |v'|: when |v'| < 0.49 h, v' is
//           the only shortest image, by a margin of 4 % that fp32 rounding cannot close, and the 27 are not tried.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr float kEps = 1.0e-12f;

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3 scale(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }

constexpr int kBoxWords = 19;   // 9 box + 9 inverse + 1 validity / search radius word per frame (odd: no LDS bank pattern)

// box[9] -> w[0..8] box, w[9..17] inverse (adjugate over determinant), w[18] = -1 unless every entry is finite and the
// determinant is finite and non-zero (the inverse is then not meaningful and is not used); else (0.49 h)^2 with h the
// smallest perpendicular width of the cell: column j of the inverse is a face normal of length 1 / width_j
__device__ __forceinline__ void box_inverse(const float* __restrict__ box, float* w) {
    float b[9];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        b[i] = box[i];
        w[i] = b[i];
        finite = finite && isfinite(b[i]);
    }
    const float c00 = b[4] * b[8] - b[5] * b[7], c01 = b[5] * b[6] - b[3] * b[8], c02 = b[3] * b[7] - b[4] * b[6];
    const float det = b[0] * c00 + b[1] * c01 + b[2] * c02;
    w[9] = c00 / det;
    w[10] = (b[2] * b[7] - b[1] * b[8]) / det;
    w[11] = (b[1] * b[5] - b[2] * b[4]) / det;
    w[12] = c01 / det;
    w[13] = (b[0] * b[8] - b[2] * b[6]) / det;
    w[14] = (b[2] * b[3] - b[0] * b[5]) / det;
    w[15] = c02 / det;
    w[16] = (b[1] * b[6] - b[0] * b[7]) / det;
    w[17] = (b[0] * b[4] - b[1] * b[3]) / det;
    const float n0 = w[9] * w[9] + w[12] * w[12] + w[15] * w[15], n1 = w[10] * w[10] + w[13] * w[13] + w[16] * w[16];
    const float n2 = w[11] * w[11] + w[14] * w[14] + w[17] * w[17];
    w[18] = (finite && isfinite(det) && det != 0.0f) ? 0.2401f / fmaxf(n0, fmaxf(n1, n2)) : -1.0f;
}

// row vector times the 3x3 matrix at m
__device__ __forceinline__ V3 vec_mat(V3 v, const float* m) {
    return {v.x * m[0] + v.y * m[3] + v.z * m[6], v.x * m[1] + v.y * m[4] + v.z * m[7],
            v.x * m[2] + v.y * m[5] + v.z * m[8]};
}

template <bool kSearch>
__device__ __forceinline__ V3 minimum_image(V3 v, const float* w) {
    V3 f = vec_mat(v, w + 9);
    f = {f.x - rintf(f.x), f.y - rintf(f.y), f.z - rintf(f.z)};
    const V3 r = vec_mat(f, w);
    if (!kSearch || dot(r, r) < w[18]) return r;
    V3 best = r;
    float best_d = __builtin_inff();
    // rolled on purpose: unrolled, the three bond vectors of a dihedral cost the kernel half its occupancy
#pragma unroll 1
    for (int idx = 0; idx < 27; ++idx) {
        const float i = (float)(idx / 9 - 1), j = (float)((idx / 3) % 3 - 1), k = (float)(idx % 3 - 1);
        V3 c = {r.x + (i * w[0] + j * w[3] + k * w[6]), r.y + (i * w[1] + j * w[4] + k * w[7]),
                r.z + (i * w[2] + j * w[5] + k * w[8])};
        if (idx == 13) c = r;
        const float d = dot(c, c);
        if (d < best_d) { best_d = d; best = c; }
    }
    return best;
}

}  // namespace
