// Frozen BatchNorm after a convolution, backward (freeze_bn fine-tuning: MODEL.USE_BN False, solver/build.py:71-76 of the
// reference).  The statistics are the running buffers and never change; gamma and beta still learn.
//
// The forward runs ONE convolution on folded operands (cr_fold_bn): wf = w * s, bias = beta - mean * s with
// s = gamma * rsqrt(var + eps), residual and ReLU in its epilogue -- the raw convolution output is never written.  The
// backward of that convolution (upstream g = dout masked by the ReLU) gives, with the existing kernels,
//   dx  = conv_bwd_data(g, wf^T)
//   dwf = conv_bwd_weight(g, x)            (f32 scratch)        sg = sum_p g   (its fused bias gradient)
// and this kernel turns (dwf, sg) into the gradients of the layer's parameters, per output channel c:
//   dw[c][:]  (+)= s_c * dwf[c][:]
//   dbeta[c]   += sg_c
//   dgamma[c]  += rsqrt(var_c + eps) * (<dwf[c], w[c]> - mean_c * sg_c)
// since <dwf[c], w[c]> = sum_p g * conv(x, w)[c] = sum_p g * y_raw.  Nothing waits on a reduction over the pixels before
// dx can be formed.  One workgroup per channel, the dot product in double in a fixed order (no atomics): bitwise
// reproducible, and the subtraction in the dgamma line loses nothing beyond the rounding of dwf itself.
#include "cr_common.h"

#define UNFOLD_T 256

__global__ __launch_bounds__(UNFOLD_T) void k_bn_frozen_unfold(const float* dwf, const float* __restrict__ sg,
                                                               const float* __restrict__ w, const float* __restrict__ gamma,
                                                               const float* __restrict__ mean, const float* __restrict__ var,
                                                               float eps, float* dw, int accumulate,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta, int K) {
    __shared__ double red[UNFOLD_T];
    const int c = blockIdx.x, t = threadIdx.x;
    const float invstd = rsqrtf(var[c] + eps);
    const float s = gamma[c] * invstd;
    const size_t row = (size_t)c * K;
    double dot = 0.0;
    // dw may alias dwf (accumulate = 0: the scaled gradient replaces the scratch in place); every element is read and
    // written by the same thread
    for (int i = t; i < K; i += UNFOLD_T) {
        const float d = dwf[row + i];
        dot += (double)d * (double)w[row + i];
        if (dw) dw[row + i] = accumulate ? dw[row + i] + s * d : s * d;
    }
    red[t] = dot;
    __syncthreads();
    for (int off = UNFOLD_T / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t == 0) {
        const double g = (double)sg[c];
        dgamma[c] += (float)((double)invstd * (red[0] - (double)mean[c] * g));
        dbeta[c] += (float)g;
    }
}

extern "C" int cr_bn_frozen_unfold(cr_ctx* ctx, const float* dwf, const float* sg, const float* w, const float* gamma,
                                   const float* mean, const float* var, float eps, float* dw, int accumulate, float* dgamma,
                                   float* dbeta, int Cout, int K) {
    CR_CHECK_ARG(ctx && dwf && sg && w && gamma && mean && var && dgamma && dbeta, "cr_bn_frozen_unfold: NULL pointer");
    CR_CHECK_ARG(Cout > 0 && K > 0, "cr_bn_frozen_unfold: bad dims Cout=%d K=%d", Cout, K);
    CR_CHECK_ARG(!(accumulate && dw == dwf), "cr_bn_frozen_unfold: dw may alias dwf only with accumulate = 0");
    hipLaunchKernelGGL(k_bn_frozen_unfold, dim3((unsigned)Cout), dim3(UNFOLD_T), 0, ctx->stream, dwf, sg, w, gamma, mean, var,
                       eps, dw, accumulate, dgamma, dbeta, K);
    CR_LAUNCH_CHECK();
    return CR_OK;
}
