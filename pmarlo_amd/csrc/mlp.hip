// Forward pass of a trained DeepTICA network (msm_mlp_forward): scaler, LayerNorm, Linear layers and activations
// for all frames in one launch, fp64 on the matrix cores.  The law and its reference operators: include/msmhip.h.
//
// A workgroup is one wave, and it owns 16 frames at a time.  Their activation rows sit in LDS as fp64 [16][stride],
// two images that the layers ping-pong between (the first as wide as the widest input of an even layer, the second
// of an odd one); nothing but the input rows is read from and nothing but the output rows written to global memory
// per frame.  As many waves as the LDS holds images for are resident per CU, and while one is in its LayerNorm and
// activation phase another has the matrix cores.  The kernel is the shared forward walk (mlp_load_inputs and
// mlp_forward_walk, mlp_common.h) with nothing kept for a backward pass.
//
// A Linear layer (mlp_linear, mlp_common.h) is out' (16 columns x 16 frames) = W (16 x K) . act' (K x 16 frames) per tile of 16 output
// columns, v_mfma_f64_16x16x4_f64, four tiles (64 columns) in flight per pass over K so that one LDS read of the
// activations feeds four independent accumulator chains.  The weights come from global memory: every wave reads
// the same few hundred KB, which stay in the caches.  Operand layout as in project_mfma_kernel
// (moments.hip): lane (j, g) = (lane & 15, lane >> 4) supplies W[c0 + j][k] and act[frame j][k] for the same k, and
// acc[r] is output column c0 + g + 4 r of frame j; k-step u of a chunk of 16 takes k = k0 + 4 g + u, so a lane's
// operands of a chunk are 16 contiguous bytes of a row of W and 32 of its activation row.  Widths are padded to 16 in
// the kernel: the last, partial chunk of K feeds zeros (both operands: a stale LDS word next to a zero weight could
// be a NaN), and output columns past N are computed from a clamped row of W and never stored.
//
// Column j of a product depends on column j of the activations alone, LayerNorm and the activations work row by
// row, and no sum depends on the launch geometry: a frame's outputs are a function of that frame's inputs, bit for
// bit.  There is no barrier: a wave's LDS traffic is ordered by the hardware and WAVE_SYNC keeps the compiler from
// reordering it.
#include "mlp_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(64) void mlp_forward_kernel(
    const T* __restrict__ x, int64_t n, int64_t ld, const double* __restrict__ sc_mean,
    const double* __restrict__ sc_scale, const float* __restrict__ params, MlpPlan p, double* __restrict__ out,
    int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_smem[];
    const int lane = threadIdx.x;
    const int j = lane & 15, g = lane >> 4;
    double* img[2];
    img[0] = reinterpret_cast<double*>(mlp_smem);
    img[1] = img[0] + 16 * p.stride[0];
    const int n_out = p.width[p.n_linear];
    const int64_t n_groups = (n + 15) / 16;
    for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int64_t t0 = grp * 16;
        const int rows = (int)min<int64_t>(16, n - t0);
        WAVE_SYNC();   // the previous group's output rows have been read
        mlp_load_inputs(img[0], p.stride[0], p.width[0], lane, rows, x, ld, sc_mean, sc_scale,
                        [&](int r) { return t0 + r; });
        int bad;
        const double* cur = mlp_forward_walk<false, false>(p, params, img, lane, rows, MlpKeep{}, &bad);
        if (j < rows) {
            const double qnan = __longlong_as_double(0x7ff8000000000000ll);
            for (int c = g; c < n_out; c += 4) out[(t0 + j) * ldo + c] = bad ? qnan : cur[c];
        }
    }
}

}  // namespace

extern "C" {

msm_status msm_mlp_forward(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                           const double* d_mean, const double* d_scale, int n_linear, const int32_t* h_widths,
                           int activation, int ln_in, int ln_hidden, int head_activation, const float* d_params,
                           size_t n_params, double* d_out, int64_t ldo) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "msm_mlp_forward: bad dtype");
    MlpPlan p;
    if (msm_status st = mlp_make_plan(ctx, "msm_mlp_forward", F, n_linear, h_widths, activation, ln_in, ln_hidden,
                                      head_activation, n_params, &p))
        return st;
    const int n_out = p.width[n_linear];
    MSM_REQUIRE(ctx, n >= 0 && ld >= F && ldo >= n_out, "msm_mlp_forward: bad shape (n = %lld, ld = %lld, ldo = %lld)",
                (long long)n, (long long)ld, (long long)ldo);
    MSM_REQUIRE(ctx, (d_mean == nullptr) == (d_scale == nullptr), "msm_mlp_forward: scaler mean and scale go together");
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_x && d_params && d_out, "msm_mlp_forward: NULL pointer");

    MlpLaunch s;
    if (msm_status st = mlp_launch_shape(ctx, mlp_forward_kernel_address(dtype), p, n, &s)) return st;
#define MSM_MLP(T)                                                                                                  \
    hipLaunchKernelGGL(mlp_forward_kernel<T>, dim3(s.grid), dim3(64), s.lds, ctx->stream, (const T*)d_x, n, ld,     \
                       d_mean, d_scale, d_params, p, d_out, ldo)
    if (dtype == MSM_F32) MSM_MLP(float);
    else MSM_MLP(double);
#undef MSM_MLP
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"

const void* mlp_forward_kernel_address(msm_dtype dtype) {
    return dtype == MSM_F32 ? (const void*)mlp_forward_kernel<float> : (const void*)mlp_forward_kernel<double>;
}
