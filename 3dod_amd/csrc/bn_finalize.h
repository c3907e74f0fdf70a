// Train-mode BatchNorm statistics finalisation shared by csrc/conv.hip (cr_bn_fwd) and csrc/resnet.hip (cr_bn_pair_fwd):
// device functions only, so that both files compile the SAME expressions in the same order -- mean / invstd and the running
// statistics of the two entry points agree bit for bit (tests/test_gpu_bn_finalize_order.py pins the order for cr_bn_fwd).
#pragma once
#include "cr_elem.h"

// at most this many statistics rows take the fused finalize + apply (k_bn_apply_fused): the 64x64 and smaller maps
static constexpr int BN_FUSE_ROWS = 256;
// from this many statistics rows on the unfused finalize runs as k_bn_stats_lanes + k_bn_finalize_lanes
static constexpr int BN_LANES_MIN_ROWS = 2048;
static constexpr int BN_LANE_BATCH = 8;     // loads in flight per thread in bn_lane_column_sum (the additions stay in row order)

// finalize: per-tile partials [nparts][2][C] -> mean / invstd (+ running stats update, momentum, unbiased var).
// One workgroup per channel; strided serial sums + a fixed-order LDS tree, in double: reproducible and accurate
// (no E[x^2]-E[x]^2 cancellation at float precision).
// bn_finalize_tail: the 256 lane sums (s, q) of channel c -> the 128 -> 1 tree and the final arithmetic (the whole block calls it)
__device__ __forceinline__ void bn_finalize_tail(double s, double q, int c, int C, float count, float eps, float momentum,
                                                 float* __restrict__ mean_invstd, float* __restrict__ running_mean,
                                                 float* __restrict__ running_var) {
    __shared__ double ss[256], sq[256];
    const int t = threadIdx.x;
    ss[t] = s; sq[t] = q;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { ss[t] += ss[t + off]; sq[t] += sq[t + off]; }
        __syncthreads();
    }
    if (t == 0) {
        // the fused multiply-adds are the ones the compiler formed from the plain expressions, now written out (the order is
        // part of what tests/test_gpu_bn_finalize_order.py specifies)
#pragma clang fp contract(off)
        const double mean = ss[0] / (double)count;
        double var = __builtin_fma(-mean, mean, sq[0] / (double)count);
        if (var < 0.0) var = 0.0;
        mean_invstd[c] = (float)mean;
        mean_invstd[C + c] = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean) {
            const double unbiased = count > 1.f ? var * (double)count / ((double)count - 1.0) : var;
            running_mean[c] = (float)__builtin_fma((double)momentum, mean, (1.0 - momentum) * running_mean[c]);
            running_var[c] = (float)__builtin_fma((double)momentum, unbiased, (1.0 - momentum) * running_var[c]);
        }
    }
}

// the sums thread t of a 256-thread workgroup forms for channel c in the one-launch finalize: rows t, t + 256, ... ascending
__device__ __forceinline__ void bn_strided_row_sums(const float* __restrict__ stats, int nparts, int C, int c, int t, double& s,
                                                    double& q) {
    s = 0.0; q = 0.0;
    for (int r = t; r < nparts; r += 256) {
        s += (double)stats[(size_t)r * 2 * C + c];
        q += (double)stats[(size_t)r * 2 * C + C + c];
    }
}

// step 1 of the two-launch finalize: flat index f = t * C2 + j (row lane t of 256, column j of C2 = 2C) -> rows t, t + 256, ...
// of column j added ascending in double: the sum bn_strided_row_sums forms for that column, bit for bit
__device__ __forceinline__ double bn_lane_column_sum(const float* __restrict__ stats, int nparts, int C2, int f) {
    const int t = f / C2, j = f - t * C2;
    const float* p = stats + (size_t)t * C2 + j;
    const size_t step = (size_t)256 * C2;
    double s = 0.0;
    int r = t;
    for (; r + 256 * (BN_LANE_BATCH - 1) < nparts; r += 256 * BN_LANE_BATCH) {
        float v[BN_LANE_BATCH];
#pragma unroll
        for (int u = 0; u < BN_LANE_BATCH; ++u) v[u] = p[(size_t)u * step];
#pragma unroll
        for (int u = 0; u < BN_LANE_BATCH; ++u) s += (double)v[u];
        p += BN_LANE_BATCH * step;
    }
    for (; r < nparts; r += 256) { s += (double)*p; p += step; }
    return s;
}

// The forward's value before the residual and the ReLU, in the one form every kernel uses: subtract, multiply, then ONE
// fused multiply-add (what the compiler made of the plain expression, now pinned).  The backward of a ReLU layer without a
// residual recomputes it from x to get the ReLU mask instead of reading the forward's output, so the bits must agree.
__device__ __forceinline__ float bn_affine(float x, float mean, float invstd, float gamma, float beta) {
#pragma clang fp contract(off)
    const float xh = (x - mean) * invstd;
    return __builtin_fmaf(xh, gamma, beta);
}

// The finalize of the fused route (few statistics rows): a 256-thread workgroup reduces the partial rows of the 32 channels
// from cbase on (8 row lanes per channel, double accumulation, fixed order: every workgroup of a slice computes the same bits)
// and leaves mean / invstd of the slice in sc[0] / sc[1].  `publish` (block-uniform): also write mean_invstd and update the
// running statistics.  The whole workgroup calls it; the caller synchronises before it reads sc (and before sd is reused).
__device__ __forceinline__ void bn_slice_finalize(const float* __restrict__ stats, int nparts, int C, int cbase, float count,
                                                  float eps, float momentum, bool publish, float* __restrict__ mean_invstd,
                                                  float* __restrict__ running_mean, float* __restrict__ running_var,
                                                  double (*sd)[8][32], float (*sc)[32]) {
    const int t = threadIdx.x, ch = t & 31, rl = t >> 5;
    const int c = cbase + ch;
    {
        double s = 0.0, q = 0.0;
        for (int r = rl; r < nparts; r += 8) {
            s += (double)stats[(size_t)r * 2 * C + c];
            q += (double)stats[(size_t)r * 2 * C + C + c];
        }
        sd[0][rl][ch] = s; sd[1][rl][ch] = q;
    }
    __syncthreads();
    if (t < 32) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) { s += sd[0][r][t]; q += sd[1][r][t]; }
        const double mean = s / (double)count;
        double var = q / (double)count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float mf = (float)mean, isf = (float)(1.0 / sqrt(var + (double)eps));
        sc[0][t] = mf;
        sc[1][t] = isf;
        if (publish) {
            mean_invstd[cbase + t] = mf;
            mean_invstd[C + cbase + t] = isf;
            if (running_mean) {
                const double unbiased = count > 1.f ? var * (double)count / ((double)count - 1.0) : var;
                running_mean[cbase + t] = (float)((1.0 - momentum) * running_mean[cbase + t] + momentum * mean);
                running_var[cbase + t] = (float)((1.0 - momentum) * running_var[cbase + t] + momentum * unbiased);
            }
        }
    }
}
