// Rigid-body superposition of every frame onto a reference (mdtraj's Trajectory.superpose) and the RMSD to it.
//
// Per frame: centroid c of the selected atoms, their 3 x 3 correlation with the centred reference and the two sums of
// squares in fp64 (two passes over the S selected atoms: centroid first, centred moments second); the proper rotation
// from Horn's quaternion matrix by bounded cyclic Jacobi (horn.h), ONE FRAME PER LANE; then out = R (x - c) + c_ref
// for all A atoms in fp32.  Memory-bound: 24 A bytes per frame with the output, 12 S without.
//
// Three kernels, picked by (A, S, which outputs) alone -- the constants are MSM_SUPERPOSE_* in msmhip.h:
//   tile    A <= LDS_ATOMS: a workgroup copies min(TILE_FRAMES, TILE_FLOATS / 3A) >= 1 consecutive frames (one
//           contiguous range of xyz) into LDS with 16-byte loads, accumulates from LDS, solves the tile's frames one
//           per lane, transforms the tile in place in LDS and copies it out with 16-byte stores: xyz is read once and
//           written once, both fully coalesced.
//   stream  A > LDS_ATOMS: a workgroup per frame; the selected atoms are gathered from global memory, and the apply
//           pass reads the frame a second time (from L2 for any frame that misses LDS by less than two orders).
//   rmsd    no output coordinates: only the selected atoms are gathered; a workgroup accumulates 256 frames into
//           LDS, then every thread solves one.
// The accumulate pass runs on 8 lanes per frame for S <= NARROW_SEL and on a whole wave above; lane g adds the atoms
// s = g, g + lanes, ... in ascending order and the lanes are combined by the DPP butterfly of wave.h, so the moments
// -- and with them the rotation and the RMSD -- have the same bits in all three kernels.
#include "common.h"
#include "horn.h"
#include "wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kStat = 16;      // doubles per frame between the passes: m[9], g_x, c[3] (+ 3 pad)
constexpr int kFit = 12;       // floats per frame for the apply pass: R[9], c[3]

template <int LANES>
__device__ __forceinline__ double group_sum(double v) {
    if constexpr (LANES == 8) return row8_reduce(v, op_sum{});
    else return wave_sum_all(v);
}

struct RefStats { double c[3], g; };

// centroid and centred sum of squares of the reference; every lane of the calling WAVE gets the same bits
__device__ __forceinline__ RefStats reference_stats(const float* __restrict__ ref, int S, int lane) {
    RefStats r;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int s = lane; s < S; s += 64) { sx += ref[3 * s]; sy += ref[3 * s + 1]; sz += ref[3 * s + 2]; }
    r.c[0] = wave_sum_all(sx) / S;
    r.c[1] = wave_sum_all(sy) / S;
    r.c[2] = wave_sum_all(sz) / S;
    double g = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double dx = ref[3 * s] - r.c[0], dy = ref[3 * s + 1] - r.c[1], dz = ref[3 * s + 2] - r.c[2];
        g += dx * dx + dy * dy + dz * dz;
    }
    r.g = wave_sum_all(g);
    return r;
}

// Moments of one frame (`fr` points at its atom 0, in LDS or global memory) on an aligned group of LANES lanes, g the
// lane's rank in it; all lanes of the group are active.  Lane g == 0 stores the kStat doubles.
template <int LANES>
__device__ __forceinline__ void frame_stats(const float* fr, const int32_t* __restrict__ sel, int S,
                                            const float* __restrict__ ref, const double* cref, int g, bool store,
                                            double* st) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int s = g; s < S; s += LANES) {
        const float* p = fr + 3 * (int64_t)sel[s];
        sx += p[0]; sy += p[1]; sz += p[2];
    }
    const double cx = group_sum<LANES>(sx) / S, cy = group_sum<LANES>(sy) / S, cz = group_sum<LANES>(sz) / S;
    double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gx = 0.0;
    for (int s = g; s < S; s += LANES) {
        const float* p = fr + 3 * (int64_t)sel[s];
        const double x = p[0] - cx, y = p[1] - cy, z = p[2] - cz;
        const double rx = ref[3 * s] - cref[0], ry = ref[3 * s + 1] - cref[1], rz = ref[3 * s + 2] - cref[2];
        gx += x * x + y * y + z * z;
        m[0] += x * rx; m[1] += x * ry; m[2] += x * rz;
        m[3] += y * rx; m[4] += y * ry; m[5] += y * rz;
        m[6] += z * rx; m[7] += z * ry; m[8] += z * rz;
    }
    gx = group_sum<LANES>(gx);
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = group_sum<LANES>(m[i]);
    if (store) {
#pragma unroll
        for (int i = 0; i < 9; ++i) st[i] = m[i];
        st[9] = gx; st[10] = cx; st[11] = cy; st[12] = cz;
    }
}

// One frame per calling thread: rotation and centroid for the apply pass (fit, may be null) and the RMSD (may be null).
// A frame with a non-finite selected coordinate has a non-finite g_x: NaN in every output of that frame.
__device__ __forceinline__ void solve_frame(const double* st, double g_ref, int S, float* fit, float* rmsd) {
    double m[9], R[9], lambda;
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = st[i];
    const double gx = st[9];
    if (!(fabs(gx) <= 1.0e300)) m[0] = nan("");
    horn_fit(m, &lambda, R);
    if (fit) {
#pragma unroll
        for (int i = 0; i < 9; ++i) fit[i] = (float)R[i];
        fit[9] = (float)st[10]; fit[10] = (float)st[11]; fit[11] = (float)st[12];
    }
    if (rmsd) *rmsd = (float)sqrt(fmax(0.0, (gx + g_ref - 2.0 * lambda) / S));   // fmax(0, NaN) is 0: restore it
    if (rmsd && !(lambda == lambda)) *rmsd = nanf("");
}

// out = R (x - c) + c_ref in fp32
__device__ __forceinline__ void apply_fit(const float* fit, const float* cref, float x, float y, float z, float* o) {
    const float dx = x - fit[9], dy = y - fit[10], dz = z - fit[11];
    o[0] = fmaf(fit[0], dx, fmaf(fit[1], dy, fmaf(fit[2], dz, cref[0])));
    o[1] = fmaf(fit[3], dx, fmaf(fit[4], dy, fmaf(fit[5], dz, cref[1])));
    o[2] = fmaf(fit[6], dx, fmaf(fit[7], dy, fmaf(fit[8], dz, cref[2])));
}

// Copies of `count` floats between global memory and the LDS tile.  The tile starts `mis` floats into a 16-byte
// aligned LDS region, mis = phase16(xyz range) = its offset inside its 16-byte line in floats, so the 16-byte accesses
// of the body are aligned on both sides whatever 12 A f0 is.  A global range of another phase (d_out that differs from
// d_xyz modulo 16 bytes) cannot be lined up with the same tile: it is copied float by float.
struct TileSplit { int head, body, done; };      // a tile has at most TILE_FLOATS floats: int
__device__ __forceinline__ int phase16(const float* g) { return (int)(((uintptr_t)g >> 2) & 3); }
__device__ __forceinline__ TileSplit split_tile(const float* g, int count, int mis) {
    TileSplit t;
    if (phase16(g) != mis) { t.head = 0; t.body = 0; t.done = 0; return t; }     // all of it in the scalar loop
    const int lead = (4 - mis) & 3;
    t.head = count < lead ? count : lead;
    t.body = (count - t.head) >> 2;
    t.done = t.head + 4 * t.body;
    return t;
}
__device__ __forceinline__ void load_tile(const float* g, float* tile, int count, int mis) {
    const TileSplit t = split_tile(g, count, mis);
    if ((int)threadIdx.x < t.head) tile[threadIdx.x] = g[threadIdx.x];
    const float4* g4 = reinterpret_cast<const float4*>(g + t.head);
    float4* t4 = reinterpret_cast<float4*>(tile + t.head);
    for (int i = threadIdx.x; i < t.body; i += kThreads) t4[i] = g4[i];
    for (int i = t.done + threadIdx.x; i < count; i += kThreads) tile[i] = g[i];
}
__device__ __forceinline__ void store_tile(float* g, const float* tile, int count, int mis) {
    const TileSplit t = split_tile(g, count, mis);
    if ((int)threadIdx.x < t.head) g[threadIdx.x] = tile[threadIdx.x];
    float4* g4 = reinterpret_cast<float4*>(g + t.head);
    const float4* t4 = reinterpret_cast<const float4*>(tile + t.head);
    for (int i = threadIdx.x; i < t.body; i += kThreads) g4[i] = t4[i];
    for (int i = t.done + threadIdx.x; i < count; i += kThreads) g[i] = tile[i];
}

template <int LANES>
__global__ __launch_bounds__(kThreads, 3) void superpose_tile_kernel(const float* xyz, int64_t n, int A,
                                                                 const int32_t* __restrict__ sel, int S,
                                                                 const float* __restrict__ ref, int T, float* out,
                                                                 float* __restrict__ rmsd) {
    extern __shared__ double lds[];
    double* s_ref = lds;                                     // c_ref[3], g_ref
    float* s_cref = reinterpret_cast<float*>(lds + 4);       // c_ref as fp32 (4 floats)
    double* s_stat = lds + 6;                                // [T][kStat]
    float* s_fit = reinterpret_cast<float*>(s_stat + (size_t)T * kStat);   // [T][kFit]
    float* s_tile = s_fit + (((size_t)T * kFit + 3) & ~(size_t)3);         // 16-byte aligned: 3 A T + 3 floats
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        const RefStats r = reference_stats(ref, S, lane);
        if (lane == 0) {
            for (int j = 0; j < 3; ++j) { s_ref[j] = r.c[j]; s_cref[j] = (float)r.c[j]; }
            s_ref[3] = r.g;
        }
    }
    const int64_t n_tiles = (n + T - 1) / T;
    for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
        const int64_t f0 = tile_id * T;
        const int tc = n - f0 < T ? (int)(n - f0) : T;
        const int64_t base = f0 * A * 3;
        const int count = tc * A * 3;
        const int mis = phase16(xyz + base);
        float* tile = s_tile + mis;
        __syncthreads();                                     // the previous tile has left LDS; s_ref is written
        load_tile(xyz + base, tile, count, mis);
        __syncthreads();
        for (int fb = 0; fb < tc; fb += kThreads / LANES) {
            const int f = fb + (int)threadIdx.x / LANES;
            const int fc = min(f, tc - 1);                   // idle groups repeat the last frame and store nothing
            frame_stats<LANES>(tile + (size_t)fc * A * 3, sel, S, ref, s_ref, threadIdx.x % LANES,
                               f < tc && threadIdx.x % LANES == 0, s_stat + (size_t)fc * kStat);
        }
        __syncthreads();
        if ((int)threadIdx.x < tc)
            solve_frame(s_stat + (size_t)threadIdx.x * kStat, s_ref[3], S, s_fit + (size_t)threadIdx.x * kFit,
                        rmsd ? rmsd + f0 + threadIdx.x : nullptr);
        __syncthreads();
        for (int i = threadIdx.x; i < tc * A; i += kThreads) {
            float* p = tile + 3 * (size_t)i;
            apply_fit(s_fit + (size_t)(i / A) * kFit, s_cref, p[0], p[1], p[2], p);
        }
        __syncthreads();
        store_tile(out + base, tile, count, mis);
    }
}

template <int LANES>
__global__ __launch_bounds__(kThreads) void superpose_stream_kernel(const float* xyz, int64_t n, int A,
                                                                   const int32_t* __restrict__ sel, int S,
                                                                   const float* __restrict__ ref, float* out,
                                                                   float* __restrict__ rmsd) {
    __shared__ double s_ref[4];
    __shared__ double s_stat[kStat];
    __shared__ float s_fit[kFit];
    __shared__ float s_cref[4];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        const RefStats r = reference_stats(ref, S, lane);
        if (lane == 0) {
            for (int j = 0; j < 3; ++j) { s_ref[j] = r.c[j]; s_cref[j] = (float)r.c[j]; }
            s_ref[3] = r.g;
        }
    }
    for (int64_t f = blockIdx.x; f < n; f += gridDim.x) {
        const float* fr = xyz + f * A * 3;
        __syncthreads();                                     // s_ref written; the previous frame's fit is consumed
        if (threadIdx.x < 64)                                // whole wave 0, of which the first LANES lanes matter
            frame_stats<LANES>(fr, sel, S, ref, s_ref, lane % LANES, lane == 0, s_stat);
        __syncthreads();
        if (threadIdx.x == 0) solve_frame(s_stat, s_ref[3], S, s_fit, rmsd ? rmsd + f : nullptr);
        __syncthreads();
        float* o = out + f * A * 3;
        for (int a = threadIdx.x; a < A; a += kThreads) {    // in place: a thread overwrites only what it has read
            const float x = fr[3 * (int64_t)a], y = fr[3 * (int64_t)a + 1], z = fr[3 * (int64_t)a + 2];
            apply_fit(s_fit, s_cref, x, y, z, o + 3 * (int64_t)a);
        }
    }
}

template <int LANES>
__global__ __launch_bounds__(kThreads) void superpose_rmsd_kernel(const float* __restrict__ xyz, int64_t n, int A,
                                                                 const int32_t* __restrict__ sel, int S,
                                                                 const float* __restrict__ ref,
                                                                 float* __restrict__ rmsd) {
    __shared__ double s_ref[4];
    __shared__ double s_stat[kThreads * kStat];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        const RefStats r = reference_stats(ref, S, lane);
        if (lane == 0) {
            for (int j = 0; j < 3; ++j) s_ref[j] = r.c[j];
            s_ref[3] = r.g;
        }
    }
    const int64_t n_batches = (n + kThreads - 1) / kThreads;
    for (int64_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        const int64_t f0 = b * kThreads;
        const int tc = n - f0 < kThreads ? (int)(n - f0) : kThreads;
        __syncthreads();
        for (int fb = 0; fb < tc; fb += kThreads / LANES) {
            const int f = fb + (int)threadIdx.x / LANES;
            const int fc = min(f, tc - 1);
            frame_stats<LANES>(xyz + (f0 + fc) * A * 3, sel, S, ref, s_ref, threadIdx.x % LANES,
                               f < tc && threadIdx.x % LANES == 0, s_stat + (size_t)fc * kStat);
        }
        __syncthreads();
        if ((int)threadIdx.x < tc)
            solve_frame(s_stat + (size_t)threadIdx.x * kStat, s_ref[3], S, nullptr, rmsd + f0 + threadIdx.x);
    }
}

}  // namespace

extern "C" msm_status msm_superpose(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const int32_t* d_sel, int S,
                                    const float* d_ref, float* d_out, float* d_rmsd) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n >= 0 && A >= 1, "msm_superpose: need n >= 0 and A >= 1 (n=%lld, A=%d)", (long long)n, A);
    MSM_REQUIRE(ctx, S >= 1 && S <= A, "msm_superpose: need 1 <= S <= A (S=%d, A=%d)", S, A);
    MSM_REQUIRE(ctx, d_out || d_rmsd, "msm_superpose: at least one of d_out / d_rmsd is needed");
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_xyz && d_sel && d_ref, "msm_superpose: NULL pointer");
    const bool narrow = S <= MSM_SUPERPOSE_NARROW_SEL;
    const int max_grid = ctx->n_cu * 8;
    if (!d_out) {
        const int grid = (int)std::min<int64_t>((n + kThreads - 1) / kThreads, max_grid);
        if (narrow)
            hipLaunchKernelGGL(superpose_rmsd_kernel<8>, dim3(grid), dim3(kThreads), 0, ctx->stream, d_xyz, n, A, d_sel,
                               S, d_ref, d_rmsd);
        else
            hipLaunchKernelGGL(superpose_rmsd_kernel<64>, dim3(grid), dim3(kThreads), 0, ctx->stream, d_xyz, n, A, d_sel,
                               S, d_ref, d_rmsd);
    } else if (A > MSM_SUPERPOSE_LDS_ATOMS) {
        const int grid = (int)std::min<int64_t>(n, max_grid);
        if (narrow)
            hipLaunchKernelGGL(superpose_stream_kernel<8>, dim3(grid), dim3(kThreads), 0, ctx->stream, d_xyz, n, A,
                               d_sel, S, d_ref, d_out, d_rmsd);
        else
            hipLaunchKernelGGL(superpose_stream_kernel<64>, dim3(grid), dim3(kThreads), 0, ctx->stream, d_xyz, n, A,
                               d_sel, S, d_ref, d_out, d_rmsd);
    } else {
        const int T = std::min(MSM_SUPERPOSE_TILE_FRAMES, MSM_SUPERPOSE_TILE_FLOATS / (3 * A));
        const int64_t n_tiles = (n + T - 1) / T;
        const int grid = (int)std::min<int64_t>(n_tiles, max_grid);
        const size_t fit_floats = ((size_t)T * kFit + 3) & ~(size_t)3;
        const size_t lds = (6 + (size_t)T * kStat) * sizeof(double) + (fit_floats + (size_t)3 * A * T + 4) * sizeof(float);
        if (narrow)
            hipLaunchKernelGGL(superpose_tile_kernel<8>, dim3(grid), dim3(kThreads), lds, ctx->stream, d_xyz, n, A, d_sel,
                               S, d_ref, T, d_out, d_rmsd);
        else
            hipLaunchKernelGGL(superpose_tile_kernel<64>, dim3(grid), dim3(kThreads), lds, ctx->stream, d_xyz, n, A,
                               d_sel, S, d_ref, T, d_out, d_rmsd);
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}
