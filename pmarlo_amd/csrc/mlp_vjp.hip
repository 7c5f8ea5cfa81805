// Gradient of a DeepTICA network's outputs with respect to its inputs (msm_mlp_vjp), and on top of it the bias
// potential of a trained network (msm_bias_energy_forces).  The law: include/msmhip.h.
//
// One launch does both passes.  As in mlp.hip a workgroup is one wave that owns 16 frames whose rows sit in two LDS
// images.  The forward pass is the shared walk (mlp_forward_walk, mlp_common.h: the outputs agree with
// mlp_forward_kernel's bit for bit) with the tape switched on: per frame, in the workspace, what the adjoints need
// (MlpTape: z, u[l], h[l]; not a[l], which only parameter gradients read).  The backward pass of the same 16 frames
// follows at once, so the tape comes back from L2: the shared adjoints (mlp_layer_adjoint, mlp_linear_transposed) with
// nothing stored for parameter gradients, carried on past the first Linear (dA_0 = du_0 . W_0), through the input
// LayerNorm, to dx = dZ / scale (the fp32 rounding of Z is the identity for the derivative).
//
// The wave reads tape rows that other lanes of it wrote to global memory; WAVE_SYNC's wavefront-scope fence orders
// them.  Nothing depends on the launch geometry: a frame's results are a function of that frame's inputs, bit for bit.
#include "mlp_common.h"

namespace {

// the workspace is the tape of the n frames; a network without one still gets a pointer to something
size_t vjp_tape_bytes(const MlpPlan& p, int64_t n, MlpTape* lay) {
    return (size_t)std::max(mlp_tape_layout(p, n, lay), 1LL) * sizeof(double);
}

template <typename T>
__global__ __launch_bounds__(64, 2) void mlp_vjp_kernel(
    const T* __restrict__ x, int64_t n, int64_t ld, const double* __restrict__ sc_mean,
    const double* __restrict__ sc_scale, const float* __restrict__ params, MlpPlan p,
    const double* __restrict__ gup, int64_t ldgo, double strength, double* __restrict__ energy,
    double* __restrict__ out, int64_t ldo, double* __restrict__ gx, int64_t ldgx, MlpTape lay, double* ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_smem[];
    const int lane = threadIdx.x;
    const int j = lane & 15, g = lane >> 4;
    double* img[2];
    img[0] = reinterpret_cast<double*>(mlp_smem);
    img[1] = img[0] + 16 * p.stride[0];
    const int F = p.width[0];
    const int L = p.n_linear;
    const int n_out = p.width[L];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int64_t n_groups = (n + 15) / 16;
    for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int64_t t0 = grp * 16;
        const int rows = (int)min<int64_t>(16, n - t0);
        const bool mine = j < rows;                               // frame j exists
        const int64_t t = min<int64_t>(t0 + j, n - 1);            // reads of a frame past n are clamped, its writes dropped
        WAVE_SYNC();   // the previous group's rows have been read
        // ---- forward, with the tape; `bad`, a non-finite Z anywhere in the frame: everything of the frame is NaN ----
        mlp_load_inputs(img[0], p.stride[0], F, lane, rows, x, ld, sc_mean, sc_scale, [&](int r) { return t0 + r; });
        int bad;
        double* cur = mlp_forward_walk<true, false>(p, params, img, lane, rows,
                                                    MlpKeep{&lay, nullptr, nullptr, ws, (size_t)t0}, &bad);
        // ---- outputs, energy, and the upstream gradient in place of the outputs ----
        double e = 0.0;
        for (int c = g; c < n_out; c += 4) e += cur[c] * cur[c];
        e = xrow_reduce(e, op_sum{});
        if (mine) {
            if (out)
                for (int c = g; c < n_out; c += 4) out[t * ldo + c] = bad ? qnan : cur[c];
            if (energy && g == 0) energy[t] = bad ? qnan : strength * e;
        }
        for (int c = g; c < n_out; c += 4)
            cur[c] = !mine ? 0.0 : (gup ? gup[t * ldgo + c] : 2.0 * strength * cur[c]);
        // ---- backward: the adjoints of every layer, carried on past the first Linear to the inputs ----
        for (int l = L - 1; l >= 0; --l) {
            double* gout = img[(l + 1) & 1] + j * p.stride[(l + 1) & 1];   // dE/d(output of layer l), then du_l
            double* gin = img[l & 1] + j * p.stride[l & 1];                // dE/d(input of layer l)
            WAVE_SYNC();   // the tape rows are in place, and so are the entries of gout other lanes wrote
            mlp_layer_adjoint<false>(gout, g, p, l, params, lay, nullptr, ws, (size_t)t, false);
            WAVE_SYNC();
            mlp_linear_transposed(gout, gin, params + p.w_off[l], p.width[l], p.width[l + 1], j, g);
        }
        double* gin = img[0] + j * p.stride[0];
        if (p.ln_in_off >= 0) {
            WAVE_SYNC();
            mlp_layer_norm_adjoint(gin, g, F, ws + lay.z + (size_t)t * F, params + p.ln_in_off, nullptr, nullptr, false);
        }
        if (mine)
            for (int f = g; f < F; f += 4) {
                const double d = sc_scale ? gin[f] / sc_scale[f] : gin[f];
                gx[t * ldgx + f] = bad ? qnan : d;
            }
    }
}

size_t feature_bytes(int64_t n, int F) { return (((size_t)n * F * sizeof(float)) + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

size_t msm_mlp_vjp_workspace(int64_t n, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                             int head_activation) {
    if (!h_widths || n < 0 || n > ((int64_t)1 << 40)) return 0;
    MlpPlan p;   // a refusal has nowhere to leave its message (no context): it is reported as 0
    if (mlp_make_plan(nullptr, "msm_mlp_vjp_workspace", h_widths[0], n_linear, h_widths, 0, ln_in, ln_hidden,
                      head_activation, kMlpAnyParams, &p))
        return 0;
    MlpTape lay;
    return vjp_tape_bytes(p, n, &lay);
}

msm_status msm_mlp_vjp(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                       const double* d_mean, const double* d_scale, int n_linear, const int32_t* h_widths,
                       int activation, int ln_in, int ln_hidden, int head_activation, const float* d_params,
                       size_t n_params, const double* d_gout, int64_t ldgo, double strength, double* d_energy,
                       double* d_out, int64_t ldo, double* d_gx, int64_t ldgx, double* d_work, size_t work_bytes) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "msm_mlp_vjp: bad dtype");
    MlpPlan p;
    if (msm_status st = mlp_make_plan(ctx, "msm_mlp_vjp", F, n_linear, h_widths, activation, ln_in, ln_hidden,
                                      head_activation, n_params, &p))
        return st;
    const int n_out = p.width[n_linear];
    MSM_REQUIRE(ctx, n >= 0 && ld >= F && ldgx >= F, "msm_mlp_vjp: bad shape (n = %lld, ld = %lld, ldgx = %lld)",
                (long long)n, (long long)ld, (long long)ldgx);
    MSM_REQUIRE(ctx, (!d_out || ldo >= n_out) && (!d_gout || ldgo >= n_out),
                "msm_mlp_vjp: row stride %lld / %lld for %d outputs", (long long)ldo, (long long)ldgo, n_out);
    MSM_REQUIRE(ctx, (d_mean == nullptr) == (d_scale == nullptr), "msm_mlp_vjp: scaler mean and scale go together");
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_x && d_params && d_gx && d_work, "msm_mlp_vjp: NULL pointer");
    MlpTape lay;
    const size_t tape = vjp_tape_bytes(p, n, &lay);
    MSM_REQUIRE(ctx, work_bytes >= tape, "msm_mlp_vjp: workspace of %zu bytes, %zu are needed", work_bytes, tape);

    MlpLaunch s;
    if (msm_status st = mlp_launch_shape(ctx, mlp_vjp_kernel_address(dtype), p, n, &s)) return st;
#define MSM_MLP_VJP(T)                                                                                               \
    hipLaunchKernelGGL(mlp_vjp_kernel<T>, dim3(s.grid), dim3(64), s.lds, ctx->stream, (const T*)d_x, n, ld, d_mean,  \
                       d_scale, d_params, p, d_gout, ldgo, strength, d_energy, d_out, ldo, d_gx, ldgx, lay, d_work)
    if (dtype == MSM_F32) MSM_MLP_VJP(float);
    else MSM_MLP_VJP(double);
#undef MSM_MLP_VJP
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

size_t msm_bias_workspace(int64_t n, int F, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                          int head_activation) {
    if (!h_widths || F != h_widths[0] || n < 0) return 0;
    const size_t tape = msm_mlp_vjp_workspace(n, n_linear, h_widths, ln_in, ln_hidden, head_activation);
    if (tape == 0) return 0;
    return feature_bytes(n, F) + (size_t)n * F * sizeof(double) + tape;
}

msm_status msm_bias_energy_forces(msm_ctx* ctx, const float* d_xyz, int64_t n, int A, const float* d_box, int64_t n_box,
                                  const int32_t* d_rec, const float* d_param, int n_rec, const int32_t* d_inc_ptr,
                                  const int32_t* d_inc, int mic, const double* d_mean, const double* d_scale,
                                  int n_linear, const int32_t* h_widths, int activation, int ln_in, int ln_hidden,
                                  int head_activation, const float* d_params, size_t n_params, double strength,
                                  double* d_work, size_t work_bytes, double* d_energy, double* d_cv, int64_t ldo,
                                  double* d_force) {
    if (!ctx) return MSM_ERR_INVALID;
    const char* who = "msm_bias_energy_forces";
    // everything the three steps would refuse is refused here, before the first of them launches
    MSM_REQUIRE(ctx, h_widths, "%s: NULL widths", who);
    const int F = h_widths[0];
    MlpPlan p;
    if (msm_status st = mlp_make_plan(ctx, who, F, n_linear, h_widths, activation, ln_in, ln_hidden, head_activation,
                                      n_params, &p))
        return st;
    MSM_REQUIRE(ctx, n >= 0 && A >= 1 && n_rec >= 1, "%s: need n >= 0, A >= 1, at least one record", who);
    MSM_REQUIRE(ctx, mic == MSM_MIC_ROUND || mic == MSM_MIC_SEARCH, "%s: mic must be MSM_MIC_ROUND or MSM_MIC_SEARCH, got %d",
                who, mic);
    MSM_REQUIRE(ctx, d_box ? (n_box == 1 || n_box == n) : n_box == 0,
                "%s: n_box=%lld must be 1 or n=%lld with a box, 0 without", who, (long long)n_box, (long long)n);
    MSM_REQUIRE(ctx, (d_mean == nullptr) == (d_scale == nullptr), "%s: scaler mean and scale go together", who);
    MSM_REQUIRE(ctx, !d_cv || ldo >= p.width[n_linear], "%s: row stride %lld for %d outputs", who, (long long)ldo,
                p.width[n_linear]);
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_xyz && d_rec && d_param && d_inc_ptr && d_inc && d_params && d_work && d_energy && d_force,
                "%s: NULL pointer", who);
    MSM_REQUIRE(ctx, ((uintptr_t)d_rec & 15) == 0, "%s: the record table must be 16-byte aligned", who);
    const size_t fbytes = feature_bytes(n, F), gbytes = (size_t)n * F * sizeof(double);
    MlpTape lay;
    const size_t tape = vjp_tape_bytes(p, n, &lay);
    MSM_REQUIRE(ctx, work_bytes >= fbytes + gbytes + tape, "%s: workspace of %zu bytes, %zu are needed", who, work_bytes,
                fbytes + gbytes + tape);
    float* feats = reinterpret_cast<float*>(d_work);
    double* gfeat = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(d_work) + fbytes);
    double* work = gfeat + (size_t)n * F;
    if (msm_status st = featurize_spec_launch(ctx, d_xyz, n, A, d_box, n_box, d_rec, d_param, n_rec, F, mic, feats, F, 0,
                                              true))
        return st;
    if (msm_status st = msm_mlp_vjp(ctx, feats, MSM_F32, n, F, F, d_mean, d_scale, n_linear, h_widths, activation, ln_in,
                                    ln_hidden, head_activation, d_params, n_params, nullptr, 0, strength, d_energy, d_cv,
                                    ldo, gfeat, F, work, tape))
        return st;
    return msm_featurize_spec_vjp(ctx, d_xyz, n, A, d_box, n_box, d_rec, d_param, n_rec, F, mic, gfeat, F, 0, d_inc_ptr,
                                  d_inc, -1.0, d_force);
}

}  // extern "C"

const void* mlp_vjp_kernel_address(msm_dtype dtype) {
    return dtype == MSM_F32 ? (const void*)mlp_vjp_kernel<float> : (const void*)mlp_vjp_kernel<double>;
}
