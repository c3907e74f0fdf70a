// ResNet-50/101 trunk kernels (cubercnn/modeling/backbone/resnet.py of the reference takes torchvision's Bottleneck): the
// projection-shortcut tail of each stage's first block,
//     out = relu( bn_a(ya) + bn_b(yb) ),   ya = conv3(t), yb = downsample conv(x), both BatchNorms in training mode,
// as ONE forward (cr_bn_pair_fwd) and ONE backward (cr_bn_pair_bwd) over the widest maps of the trunk.  Against the two-call
// composition cr_bn_fwd(yb) -> cr_bn_fwd(ya, residual, relu) the normalised shortcut is never written or read back, and the
// backward never writes the masked gradient for the second BatchNorm and reads each operand twice, not three times.
// Memory-bound vector-ALU work in plain C++: NHWC, 8 channels (16 bytes of bf16, 32 of f32) per thread, 64-bit element
// offsets, no atomics, every sum in a fixed order (the same bits on every run; there is no separate deterministic path).
// Channel domain of cr_bn_bwd: C % 8 == 0, C <= 2048, 256 % (C / 8) == 0 -- a thread's channels do not change while it
// strides over pixels, so the per-channel constants live in registers.
#include "cr_common.h"
#include "cr_elem.h"
#include "bn_finalize.h"
#include "cr3dod.h"

namespace {

// one BatchNorm of the pair
struct BnSide {
    const float* stats;          // [nparts][2][C]
    const float* gamma;
    const float* beta;
    float* mean_invstd;          // [2][C]
    float* running_mean;         // may be NULL (then running_var is not touched either)
    float* running_var;
    float eps, momentum;
};

// ---- forward, at most BN_FUSE_ROWS statistics rows: finalize + apply in one launch (the plan of k_bn_apply_fused) ----------
// workgroup (pixel chunk, channel slice of 32) reduces the statistics rows of its slice for both BatchNorms with
// bn_slice_finalize -- the code cr_bn_fwd runs --, then normalises its pixels; the workgroups of chunk 0 publish mean / invstd
// and update the running statistics.
template <typename T>
__global__ __launch_bounds__(256) void k_bnp_apply_fused(const T* __restrict__ ya, const T* __restrict__ yb, const BnSide a,
                                                         const BnSide b, int nparts, float count, T* __restrict__ out,
                                                         int64_t M, int C, int px_per_block) {
    __shared__ double sd[2][8][32];
    __shared__ float sca[2][32], scb[2][32];             // mean, invstd of this slice
    const int t = threadIdx.x;
    const int cbase = blockIdx.y * 32;
    bn_slice_finalize(b.stats, nparts, C, cbase, count, b.eps, b.momentum, blockIdx.x == 0, b.mean_invstd, b.running_mean,
                      b.running_var, sd, scb);
    __syncthreads();                                     // sd is free again
    bn_slice_finalize(a.stats, nparts, C, cbase, count, a.eps, a.momentum, blockIdx.x == 0, a.mean_invstd, a.running_mean,
                      a.running_var, sd, sca);
    __syncthreads();
    const int cgl = t & 3;                               // 8-channel group inside the slice
    float mua[8], isa[8], gaa[8], bea[8], mub[8], isb[8], gab[8], beb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int cc = cgl * 8 + e;
        mua[e] = sca[0][cc]; isa[e] = sca[1][cc]; gaa[e] = a.gamma[cbase + cc]; bea[e] = a.beta[cbase + cc];
        mub[e] = scb[0][cc]; isb[e] = scb[1][cc]; gab[e] = b.gamma[cbase + cc]; beb[e] = b.beta[cbase + cc];
    }
    const int64_t m0 = (int64_t)blockIdx.x * px_per_block, m1 = m0 + px_per_block < M ? m0 + px_per_block : M;
    for (int64_t m = m0 + (t >> 2); m < m1; m += 64) {
        const size_t i8 = (size_t)m * C + cbase + cgl * 8;
        float xa[8], xb[8], o[8];
        load8<T>(ya, i8, xa);
        load8<T>(yb, i8, xb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float idn = bn_affine(xb[e], mub[e], isb[e], gab[e], beb[e]);      // the shortcut, never stored
            float v = bn_affine(xa[e], mua[e], isa[e], gaa[e], bea[e]);
            v += idn;                                                                // as k_bn_apply adds its residual
            o[e] = fmaxf(v, 0.f);
        }
        store8<T>(out, i8, o);
    }
}

// ---- forward, more rows: the finalize kernels of cr_bn_fwd for both BatchNorms in one launch each (blockIdx.y = which) -----
__global__ __launch_bounds__(256) void k_bnp_finalize(const BnSide a, const BnSide b, int nparts, int C, float count) {
    const BnSide& s = blockIdx.y ? b : a;
    const int c = blockIdx.x, t = threadIdx.x;
    double sum, sq;
    bn_strided_row_sums(s.stats, nparts, C, c, t, sum, sq);
    bn_finalize_tail(sum, sq, c, C, count, s.eps, s.momentum, s.mean_invstd, s.running_mean, s.running_var);
}

// lanes: [2][256][2C] doubles
__global__ __launch_bounds__(256) void k_bnp_stats_lanes(const float* __restrict__ stats_a, const float* __restrict__ stats_b,
                                                         int nparts, int C2, double* __restrict__ lanes) {
    const int f = blockIdx.x * 256 + threadIdx.x;         // < 256 * C2 (grid.x = C2 blocks)
    lanes[(size_t)blockIdx.y * 256 * C2 + f] = bn_lane_column_sum(blockIdx.y ? stats_b : stats_a, nparts, C2, f);
}

__global__ __launch_bounds__(256) void k_bnp_finalize_lanes(const double* __restrict__ lanes, const BnSide a, const BnSide b,
                                                            int C, float count) {
    const BnSide& s = blockIdx.y ? b : a;
    const int c = blockIdx.x, t = threadIdx.x;
    const double* l = lanes + (size_t)blockIdx.y * 256 * 2 * C;
    bn_finalize_tail(l[(size_t)t * 2 * C + c], l[(size_t)t * 2 * C + C + c], c, C, count, s.eps, s.momentum, s.mean_invstd,
                     s.running_mean, s.running_var);
}

// out = relu(bn_affine(ya) + bn_affine(yb)) from the published mean / invstd.  The grid's thread count is a multiple of C / 8,
// so thread i owns the channels (i % (C / 8)) * 8 .. + 7 of every pixel it visits.
template <typename T>
__global__ __launch_bounds__(256) void k_bnp_apply(const T* __restrict__ ya, const T* __restrict__ yb,
                                                   const float* __restrict__ mia, const float* __restrict__ mib,
                                                   const float* __restrict__ gamma_a, const float* __restrict__ beta_a,
                                                   const float* __restrict__ gamma_b, const float* __restrict__ beta_b,
                                                   T* __restrict__ out, int64_t M, int C) {
    const int cg = C >> 3;
    const int64_t total = M * cg;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c0 = (int)(i0 % cg) << 3;
    float mua[8], isa[8], gaa[8], bea[8], mub[8], isb[8], gab[8], beb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        mua[e] = mia[c0 + e]; isa[e] = mia[C + c0 + e]; gaa[e] = gamma_a[c0 + e]; bea[e] = beta_a[c0 + e];
        mub[e] = mib[c0 + e]; isb[e] = mib[C + c0 + e]; gab[e] = gamma_b[c0 + e]; beb[e] = beta_b[c0 + e];
    }
    for (int64_t i = i0; i < total; i += (int64_t)gridDim.x * 256) {
        float xa[8], xb[8], o[8];
        load8<T>(ya, (size_t)i * 8, xa);
        load8<T>(yb, (size_t)i * 8, xb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float idn = bn_affine(xb[e], mub[e], isb[e], gab[e], beb[e]);
            float v = bn_affine(xa[e], mua[e], isa[e], gaa[e], bea[e]);
            v += idn;
            o[e] = fmaxf(v, 0.f);
        }
        store8<T>(out, (size_t)i * 8, o);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// g = dout * [out > 0], xh = (y - mean) * invstd.  Per channel: S0 = sum g (both dbeta), Sa = sum g * xh_a, Sb = sum g * xh_b;
//   dxa_raw = gamma_a * invstd_a * (g - S0 / M - xh_a * Sa / M), the same for b.
// pass 1: workgroup bx takes the rows bx * rpb + myrow + k * gridDim.x * rpb (rpb = 256 / (C / 8) rows of 8-channel threads); a
// thread adds its few rows in float32 (the launcher sizes the grid for 8 rows while it has workgroups left), the rpb row
// threads of a channel are added in row order in double through LDS -> partial[bx][3][C].
#define BNP_MAXBLOCKS 1024
template <typename T>
__global__ __launch_bounds__(256) void k_bnp_bwd_reduce(const T* __restrict__ dout, const T* __restrict__ out,
                                                        const T* __restrict__ ya, const T* __restrict__ yb,
                                                        const float* __restrict__ mia, const float* __restrict__ mib,
                                                        float* __restrict__ partial, int64_t M, int C) {
    __shared__ float s_acc[2048];           // [rpb][C]: 256 / cg rows of 8 * cg channels
    const int cg = C >> 3;
    const int t = threadIdx.x, mycg = t % cg, myrow = t / cg;
    const int rpb = 256 / cg;
    const int c0 = mycg << 3;
    float acc[3][8], mua[8], isa[8], mub[8], isb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[0][e] = 0.f; acc[1][e] = 0.f; acc[2][e] = 0.f;
        mua[e] = mia[c0 + e]; isa[e] = mia[C + c0 + e]; mub[e] = mib[c0 + e]; isb[e] = mib[C + c0 + e];
    }
    for (int64_t m = (int64_t)blockIdx.x * rpb + myrow; m < M; m += (int64_t)gridDim.x * rpb) {
        const size_t i8 = (size_t)m * C + c0;
        float dv[8], ov[8], xa[8], xb[8];
        load8<T>(dout, i8, dv);
        load8<T>(out, i8, ov);
        load8<T>(ya, i8, xa);
        load8<T>(yb, i8, xb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gq = ov[e] > 0.f ? dv[e] : 0.f;
            acc[0][e] += gq;
            acc[1][e] += gq * ((xa[e] - mua[e]) * isa[e]);
            acc[2][e] += gq * ((xb[e] - mub[e]) * isb[e]);
        }
    }
    float* dst = partial + (size_t)blockIdx.x * 3 * C;
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        if (which) __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) s_acc[myrow * C + c0 + e] = acc[which][e];
        __syncthreads();
        for (int c = t; c < C; c += 256) {
            double s = 0.0;                 // the rows' sums cancel: add them in double, round once
            for (int r = 0; r < rpb; ++r) s += (double)s_acc[r * C + c];            // fixed order
            dst[which * C + c] = (float)s;
        }
    }
}

// pass 2: workgroup (channel slice of 32, which of S0 / Sa / Sb): 32 row lanes per channel add the partial rows lane, lane + 32,
// ... ascending in double, then lane order -> sums[which][C]; dgamma / dbeta accumulated (S0 goes to both dbeta)
__global__ __launch_bounds__(1024) void k_bnp_bwd_finalize(const float* __restrict__ partial, int nparts, int C,
                                                           float* __restrict__ sums, float* __restrict__ dgamma_a,
                                                           float* __restrict__ dbeta_a, float* __restrict__ dgamma_b,
                                                           float* __restrict__ dbeta_b) {
    __shared__ double sd[32][32];
    const int t = threadIdx.x, ch = t & 31, rl = t >> 5;
    const int which = blockIdx.y, c = blockIdx.x * 32 + ch;
    double s = 0.0;
    if (c < C) {
        const float* p = partial + (size_t)which * C + c;
        int r = rl;
        for (; r + 32 * 3 < nparts; r += 32 * 4) {       // four loads in flight, added in row order
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p[(size_t)(r + 32 * u) * 3 * C];
#pragma unroll
            for (int u = 0; u < 4; ++u) s += (double)v[u];
        }
        for (; r < nparts; r += 32) s += (double)p[(size_t)r * 3 * C];
    }
    sd[rl][ch] = s;
    __syncthreads();
    if (t < 32 && c < C) {
        double tot = 0.0;
        for (int r = 0; r < 32; ++r) tot += sd[r][t];    // fixed order
        const float f = (float)tot;
        sums[which * C + c] = f;
        if (which == 0) { dbeta_a[c] += f; dbeta_b[c] += f; }
        else if (which == 1) dgamma_a[c] += f;
        else dgamma_b[c] += f;
    }
}

// pass 3: both input gradients; thread i owns the channels (i % (C / 8)) * 8 .. + 7 of every pixel it visits
template <typename T>
__global__ __launch_bounds__(256) void k_bnp_bwd_apply(const T* __restrict__ dout, const T* __restrict__ out,
                                                       const T* __restrict__ ya, const T* __restrict__ yb,
                                                       const float* __restrict__ mia, const float* __restrict__ mib,
                                                       const float* __restrict__ gamma_a, const float* __restrict__ gamma_b,
                                                       const float* __restrict__ sums, T* __restrict__ dxa,
                                                       T* __restrict__ dxb, int64_t M, int C) {
    const int cg = C >> 3;
    const int64_t total = M * cg;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c0 = (int)(i0 % cg) << 3;
    const float invM = 1.f / (float)M;
    float mua[8], isa[8], sca[8], ka[8], mub[8], isb[8], scb[8], kb[8], k0[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        mua[e] = mia[c]; isa[e] = mia[C + c]; sca[e] = gamma_a[c] * isa[e]; ka[e] = sums[C + c] * invM;
        mub[e] = mib[c]; isb[e] = mib[C + c]; scb[e] = gamma_b[c] * isb[e]; kb[e] = sums[2 * C + c] * invM;
        k0[e] = sums[c] * invM;
    }
    for (int64_t i = i0; i < total; i += (int64_t)gridDim.x * 256) {
        float dv[8], ov[8], xa[8], xb[8], va[8], vb[8];
        load8<T>(dout, (size_t)i * 8, dv);
        load8<T>(out, (size_t)i * 8, ov);
        load8<T>(ya, (size_t)i * 8, xa);
        load8<T>(yb, (size_t)i * 8, xb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gq = ov[e] > 0.f ? dv[e] : 0.f;
            const float gc = gq - k0[e];
            va[e] = sca[e] * (gc - ((xa[e] - mua[e]) * isa[e]) * ka[e]);
            vb[e] = scb[e] * (gc - ((xb[e] - mub[e]) * isb[e]) * kb[e]);
        }
        store8<T>(dxa, (size_t)i * 8, va);
        store8<T>(dxb, (size_t)i * 8, vb);
    }
}

int check_pair(const char* who, int64_t M, int C, int act_f32) {
    CR_CHECK_ARG(M >= 1, "%s: M must be >= 1 (got %lld)", who, (long long)M);
    CR_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= 2048 && 256 % (C >> 3) == 0,
                 "%s: unsupported C=%d (C %% 8 == 0, C <= 2048, 256 %% (C / 8) == 0)", who, C);
    CR_CHECK_ARG(act_f32 >= 0 && act_f32 <= 2, "%s: act_f32 must be 0, 1 or 2 (got %d)", who, act_f32);
    return CR_OK;
}

// workgroups of pass 1 and rows of the partial table: 8 rows per thread while that needs at most BNP_MAXBLOCKS workgroups
int64_t pair_bwd_blocks(int64_t M, int C) {
    const int rpb = 256 / (C >> 3);
    int64_t nb = cr_cdiv(M, (int64_t)rpb * 8);
    if (nb > BNP_MAXBLOCKS) nb = BNP_MAXBLOCKS;
    return nb < 1 ? 1 : nb;
}

template <typename T>
int pair_fwd_launch(cr_ctx* ctx, const T* ya, const T* yb, const BnSide& a, const BnSide& b, int nparts, T* out, int64_t M, int C) {
    if (C % 32 == 0 && nparts <= BN_FUSE_ROWS) {
        int64_t chunks = 1024 / (C / 32);                // the grid of cr_bn_fwd's fused route
        if (chunks < 1) chunks = 1;
        int64_t ppb = cr_cdiv(M, chunks);
        ppb = (ppb + 63) / 64 * 64;
        const dim3 grid((unsigned)cr_cdiv(M, ppb), (unsigned)(C / 32));
        hipLaunchKernelGGL(k_bnp_apply_fused<T>, grid, dim3(256), 0, ctx->stream, ya, yb, a, b, nparts, (float)M, out, M, C,
                           (int)ppb);
        CR_LAUNCH_CHECK();
        return CR_OK;
    }
    const size_t lanes_bytes = sizeof(double) * 256 * 2 * C;      // per BatchNorm
    if (nparts >= BN_LANES_MIN_ROWS && ctx->ws && 2 * lanes_bytes <= ctx->ws_bytes) {
        double* lanes = (double*)ctx->ws;                // written and read by this call's two launches only
        hipLaunchKernelGGL(k_bnp_stats_lanes, dim3((unsigned)(2 * C), 2), dim3(256), 0, ctx->stream, a.stats, b.stats, nparts,
                           2 * C, lanes);
        CR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_bnp_finalize_lanes, dim3((unsigned)C, 2), dim3(256), 0, ctx->stream, lanes, a, b, C, (float)M);
    } else {
        hipLaunchKernelGGL(k_bnp_finalize, dim3((unsigned)C, 2), dim3(256), 0, ctx->stream, a, b, nparts, C, (float)M);
    }
    CR_LAUNCH_CHECK();
    const int64_t total = M * (C >> 3);
    const unsigned grid = (unsigned)(cr_cdiv(total, 256) < 4096 ? cr_cdiv(total, 256) : 4096);
    hipLaunchKernelGGL(k_bnp_apply<T>, dim3(grid), dim3(256), 0, ctx->stream, ya, yb, a.mean_invstd, b.mean_invstd, a.gamma,
                       a.beta, b.gamma, b.beta, out, M, C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

template <typename T>
int pair_bwd_launch(cr_ctx* ctx, const T* dout, const T* out, const T* ya, const T* yb, const float* mia, const float* mib,
                    const float* gamma_a, const float* gamma_b, float* ws, T* dxa, T* dxb, float* dgamma_a, float* dbeta_a,
                    float* dgamma_b, float* dbeta_b, int64_t M, int C) {
    const int64_t nb = pair_bwd_blocks(M, C);
    float* sums = ws + (size_t)nb * 3 * C;
    hipLaunchKernelGGL(k_bnp_bwd_reduce<T>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, dout, out, ya, yb, mia, mib, ws, M, C);
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bnp_bwd_finalize, dim3((unsigned)cr_cdiv(C, 32), 3), dim3(1024), 0, ctx->stream, ws, (int)nb, C, sums,
                       dgamma_a, dbeta_a, dgamma_b, dbeta_b);
    CR_LAUNCH_CHECK();
    const int64_t total = M * (C >> 3);
    const unsigned grid = (unsigned)(cr_cdiv(total, 256) < 4096 ? cr_cdiv(total, 256) : 4096);
    hipLaunchKernelGGL(k_bnp_bwd_apply<T>, dim3(grid), dim3(256), 0, ctx->stream, dout, out, ya, yb, mia, mib, gamma_a, gamma_b,
                       sums, dxa, dxb, M, C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

}  // namespace

extern "C" int cr_bn_pair_fwd(cr_ctx* ctx, const void* ya, const void* yb, const float* stats_a, const float* stats_b, int nparts,
                              const float* gamma_a, const float* beta_a, const float* gamma_b, const float* beta_b, void* out,
                              int64_t M, int C, float eps_a, float momentum_a, float eps_b, float momentum_b,
                              float* mean_invstd_a, float* mean_invstd_b, float* running_mean_a, float* running_var_a,
                              float* running_mean_b, float* running_var_b, int act_f32) {
    CR_CHECK_ARG(ctx && ya && yb && stats_a && stats_b && gamma_a && beta_a && gamma_b && beta_b && out && mean_invstd_a &&
                 mean_invstd_b, "cr_bn_pair_fwd: NULL pointer");
    if (int rc = check_pair("cr_bn_pair_fwd", M, C, act_f32)) return rc;
    CR_CHECK_ARG((int64_t)nparts == cr_cdiv(M, 64), "cr_bn_pair_fwd: %d statistics rows for M=%lld (one per 64 pixels)", nparts,
                 (long long)M);
    CR_CHECK_ARG(!running_mean_a == !running_var_a && !running_mean_b == !running_var_b,
                 "cr_bn_pair_fwd: running_mean and running_var go together");
    // the two BatchNorms are finalised side by side (blockIdx.y, or one after the other inside a workgroup): a buffer of one
    // that is also a buffer of the other would be written from both
    float* const wr[6] = {mean_invstd_a, running_mean_a, running_var_a, mean_invstd_b, running_mean_b, running_var_b};
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            CR_CHECK_ARG(!wr[i] || wr[i] != wr[j], "cr_bn_pair_fwd: mean_invstd and the running statistics need six separate buffers");
    const BnSide a = {stats_a, gamma_a, beta_a, mean_invstd_a, running_mean_a, running_var_a, eps_a, momentum_a};
    const BnSide b = {stats_b, gamma_b, beta_b, mean_invstd_b, running_mean_b, running_var_b, eps_b, momentum_b};
    if (act_f32) return pair_fwd_launch<float>(ctx, (const float*)ya, (const float*)yb, a, b, nparts, (float*)out, M, C);
    return pair_fwd_launch<u16>(ctx, (const u16*)ya, (const u16*)yb, a, b, nparts, (u16*)out, M, C);
}

// rows of the partial table of cr_bn_pair_bwd (its workspace: (rows + 1) * 3 * C floats); 0 outside the domain
extern "C" int cr_bn_pair_bwd_blocks(int64_t M, int C) {
    if (M < 1 || C < 8 || C % 8 || C > 2048 || 256 % (C >> 3)) return 0;
    return (int)pair_bwd_blocks(M, C);
}

extern "C" int cr_bn_pair_bwd(cr_ctx* ctx, const void* dout, const void* out, const void* ya, const void* yb,
                              const float* mean_invstd_a, const float* mean_invstd_b, const float* gamma_a, const float* gamma_b,
                              float* ws, int64_t ws_floats, void* dxa_raw, void* dxb_raw, float* dgamma_a, float* dbeta_a,
                              float* dgamma_b, float* dbeta_b, int64_t M, int C, int act_f32) {
    CR_CHECK_ARG(ctx && dout && out && ya && yb && mean_invstd_a && mean_invstd_b && gamma_a && gamma_b && ws && dxa_raw &&
                 dxb_raw && dgamma_a && dbeta_a && dgamma_b && dbeta_b, "cr_bn_pair_bwd: NULL pointer");
    if (int rc = check_pair("cr_bn_pair_bwd", M, C, act_f32)) return rc;
    CR_CHECK_ARG(dbeta_a != dbeta_b && dgamma_a != dgamma_b, "cr_bn_pair_bwd: the two BatchNorms need separate gradient buffers");
    const int64_t need = (pair_bwd_blocks(M, C) + 1) * 3 * C;
    CR_CHECK_ARG(ws_floats >= need, "cr_bn_pair_bwd: workspace of %lld floats, %lld needed ((blocks + 1) * 3 * C)",
                 (long long)ws_floats, (long long)need);
    if (act_f32)
        return pair_bwd_launch<float>(ctx, (const float*)dout, (const float*)out, (const float*)ya, (const float*)yb,
                                      mean_invstd_a, mean_invstd_b, gamma_a, gamma_b, ws, (float*)dxa_raw, (float*)dxb_raw,
                                      dgamma_a, dbeta_a, dgamma_b, dbeta_b, M, C);
    return pair_bwd_launch<u16>(ctx, (const u16*)dout, (const u16*)out, (const u16*)ya, (const u16*)yb, mean_invstd_a,
                                mean_invstd_b, gamma_a, gamma_b, ws, (u16*)dxa_raw, (u16*)dxb_raw, dgamma_a, dbeta_a, dgamma_b,
                                dbeta_b, M, C);
}
