// Dense-block kernels of the DenseNet-121 trunk (cubercnn/modeling/backbone/densenet.py of the reference, which takes
// torchvision's densenet121.features): everything a dense block needs besides its two convolutions.
//
// A block keeps ONE feature buffer X (M, ld) in NHWC, M = N*H*W pixels, ld = C0 + 32 * L channels, in the activation type.
// Layer i reads channels [0, C_i) and its 3x3 convolution's 32 new channels are copied to [C_i, C_i + 32).  Beside X sits a
// table tab (3, ld) f32 = batch mean | biased variance | inverse std per channel, filled ONCE per channel: a feature's
// statistics do not change when later layers read it again.  The gradient of X is accumulated in G (M, ld), ALWAYS f32: up to
// 24 layers add into one slice.
//
// All kernels are memory-bound and written in plain C++ on the storage type T in {u16 (bf16), float}:
//   * 8 channels (16 bytes of bf16, 2 x 16 bytes of f32) per access, 64-bit element offsets, every access predicated on M;
//   * channel counts are multiples of 32 (slice copies: 8), 32 <= C <= 1024 -- anything else is CR_EINVAL, never a launch;
//   * no atomics: every reduction is a partial-sum launch (a workgroup sums its pixel range of a 32-channel slice) followed by
//     a finalize launch that adds the partial rows in index order in double -> bit-identical from run to run;
//   * the ReLU mask of the backward is recomputed from X with the forward's own expression (dn_affine), as cr_bn_bwd_mask does.
#include "cr_common.h"
#include "cr_elem.h"

namespace {

constexpr int DN_CMAX = 1024;          // widest slice (denseblock3 / denseblock4 end at 1024 channels)
constexpr int DN_PARTS = 256;          // at most this many partial rows per reduction

// the value the forward stores before the ReLU: subtract, multiply, ONE fused multiply-add -- pinned, the backward recomputes it
__device__ __forceinline__ float dn_affine(float x, float mean, float invstd, float gamma, float beta) {
#pragma clang fp contract(off)
    const float xh = (x - mean) * invstd;
    return __builtin_fmaf(xh, gamma, beta);
}
template <typename T> __device__ __forceinline__ bool dn_relu_on(float v);
template <> __device__ __forceinline__ bool dn_relu_on<float>(float v) { return fmaxf(v, 0.f) > 0.f; }
template <> __device__ __forceinline__ bool dn_relu_on<u16>(float v) { return bf2f(f2bf(fmaxf(v, 0.f))) > 0.f; }
// inverse std of the running-statistics mode (eval, freeze_bn); forward and backward must agree on the bits
__device__ __forceinline__ float dn_running_invstd(float var, float eps) { return 1.0f / sqrtf(var + eps); }

static int64_t dn_rows_per_part(int64_t M) {
    int64_t r = cr_cdiv(M, DN_PARTS);
    r = (r + 63) / 64 * 64;
    return r < 64 ? 64 : r;
}

// ---------------------------------------------------------------------------------------------------------------------
// partial sums.  Workgroup (part, slice of 32 channels): thread = (8-channel group t & 3, row lane t >> 2) walks the rows of
// its part; the 64 row lanes are added in lane order.  BWD = 0: sum x, sum x^2 of X[:, c0 + .].  BWD = 1 / 2 (without / with a
// ReLU): with g = da masked by the recomputed ReLU and xh = (x - mean) * invstd: sum g, sum g * xh of X[:, .].
// part = f32 [nparts][2][C].  The ReLU is a template argument: the mask is then a plain select, with no uniform branch around it.
// ---------------------------------------------------------------------------------------------------------------------
struct DnPartP {
    const void* x; const void* da;
    const float* mean; const float* invstd;     // batch mode: rows of tab; running mode: running_mean / running_var
    const float* gamma; const float* beta;
    float* part;
    long long M, ldx;
    int C, c0, running, rows_pp;
    float eps;
};

template <typename T, int BWD>
__global__ __launch_bounds__(256) void k_dn_partial(const DnPartP p) {
    __shared__ float sm[64][2][32];
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ da = reinterpret_cast<const T*>(p.da);
    const int t = threadIdx.x, cgl = t & 3, rl = t >> 2;
    const int c = blockIdx.y * 32 + cgl * 8;                 // < C: C is a multiple of 32
    float mu[8], is8[8], ga[8], be[8];
    if (BWD) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mu[e] = p.mean[c + e];
            is8[e] = p.running ? dn_running_invstd(p.invstd[c + e], p.eps) : p.invstd[c + e];
            ga[e] = p.gamma[c + e];
            be[e] = p.beta[c + e];
        }
    }
    float s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
    const long long m0 = (long long)blockIdx.x * p.rows_pp;
    const long long m1 = m0 + p.rows_pp < p.M ? m0 + p.rows_pp : p.M;
    for (long long m = m0 + rl; m < m1; m += 64) {
        float xv[8];
        load8<T>(x, (size_t)m * p.ldx + p.c0 + c, xv);
        if (BWD) {
            float gv[8];
            load8<T>(da, (size_t)m * p.C + c, gv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = (xv[e] - mu[e]) * is8[e];
                float g = gv[e];
                if (BWD == 2) g = dn_relu_on<T>(dn_affine(xv[e], mu[e], is8[e], ga[e], be[e])) ? g : 0.f;
                s[e] += g;
                q[e] = fmaf(g, xh, q[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s[e] += xv[e];
                q[e] = fmaf(xv[e], xv[e], q[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sm[rl][0][cgl * 8 + e] = s[e];
        sm[rl][1][cgl * 8 + e] = q[e];
    }
    __syncthreads();
    if (t < 64) {
        const int which = t >> 5, ch = t & 31;
        double a = 0.0;
        for (int r = 0; r < 64; ++r) a += (double)sm[r][which][ch];
        p.part[((size_t)blockIdx.x * 2 + which) * p.C + blockIdx.y * 32 + ch] = (float)a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// finalize: workgroup = 32 channels x 8 row lanes over part [nparts][2][C], lanes added in order, in double.
// MODE 0: mean, biased variance, inverse std -> tab (3, ldt) at channel offset `off`.
// MODE 1: sums [2][C] = sum g, sum g * xh (read by the apply kernel); dbeta += sum g, dgamma += sum g * xh.
// ---------------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_dn_final(const float* __restrict__ part, int nparts, int C, double count, float eps,
                                                  float* __restrict__ tab, int ldt, int off, float* __restrict__ sums,
                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sd[2][8][32];
    const int t = threadIdx.x, ch = t & 31, rl = t >> 5;
    const int c = blockIdx.x * 32 + ch;
    double s = 0.0, q = 0.0;
    for (int r = rl; r < nparts; r += 8) {
        s += (double)part[(size_t)r * 2 * C + c];
        q += (double)part[(size_t)r * 2 * C + C + c];
    }
    sd[0][rl][ch] = s;
    sd[1][rl][ch] = q;
    __syncthreads();
    if (t < 32) {
        s = 0.0; q = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) { s += sd[0][r][t]; q += sd[1][r][t]; }
        if (MODE == 0) {
            const double mean = s / count;
            double var = q / count - mean * mean;
            if (var < 0.0) var = 0.0;
            tab[off + c] = (float)mean;
            tab[ldt + off + c] = (float)var;
            tab[2 * (size_t)ldt + off + c] = (float)(1.0 / sqrt(var + (double)eps));
        } else {
            sums[c] = (float)s;
            sums[C + c] = (float)q;
            dbeta[c] += (float)s;
            dgamma[c] += (float)q;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// a = act(gamma * (X[:, :C] - mean) * invstd + beta), contiguous (M, C).  A workgroup stages the per-channel constants in LDS
// and normalises rows_pb rows; workgroup 0 of the batch-statistics mode updates this layer's running statistics.
// ---------------------------------------------------------------------------------------------------------------------
struct DnBnP {
    const void* x; void* out;                   // forward: X -> a
    const void* da; float* G;                   // backward: da, X -> G
    const float* tab; int ldt;                  // batch mode
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;
    const float* sums;                          // backward, batch mode: [2][C]
    long long M, ldx, ldg;
    int C, relu, batch, accumulate, rows_pb;
    float eps, momentum;
};

template <typename T>
__global__ __launch_bounds__(256) void k_dn_bn_fwd(const DnBnP p) {
    __shared__ float sp[4][DN_CMAX];
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    T* __restrict__ out = reinterpret_cast<T*>(p.out);
    const int t = threadIdx.x, C = p.C, cg = C >> 3;
    for (int c = t; c < C; c += 256) {
        float mean, is;
        if (p.batch) {
            mean = p.tab[c];
            is = p.tab[2 * (size_t)p.ldt + c];
            if (blockIdx.x == 0 && p.running_mean) {
                const double cnt = (double)p.M, var = (double)p.tab[p.ldt + c];
                const double unbiased = p.M > 1 ? var * cnt / (cnt - 1.0) : var;
                const double mom = (double)p.momentum;
                p.running_mean[c] = (float)((1.0 - mom) * (double)p.running_mean[c] + mom * (double)mean);
                p.running_var[c] = (float)((1.0 - mom) * (double)p.running_var[c] + mom * unbiased);
            }
        } else {
            mean = p.running_mean[c];
            is = dn_running_invstd(p.running_var[c], p.eps);
        }
        sp[0][c] = mean; sp[1][c] = is; sp[2][c] = p.gamma[c]; sp[3][c] = p.beta[c];
    }
    __syncthreads();
    const long long m0 = (long long)blockIdx.x * p.rows_pb;
    const int rows = (int)((m0 + p.rows_pb < p.M ? m0 + p.rows_pb : p.M) - m0);
    const int items = rows * cg;
    for (int j = t; j < items; j += 256) {
        const int r = j / cg, c = (j - r * cg) << 3;
        const long long m = m0 + r;
        float xv[8], o[8];
        load8<T>(x, (size_t)m * p.ldx + c, xv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = dn_affine(xv[e], sp[0][c + e], sp[1][c + e], sp[2][c + e], sp[3][c + e]);
            o[e] = p.relu ? fmaxf(v, 0.f) : v;
        }
        store8<T>(out, (size_t)m * C + c, o);
    }
}

// G[:, :C] (+)= gamma * invstd * (g - sum g / M - xh * sum(g xh) / M); the two correction terms only in batch mode
template <typename T, bool RELU>
__global__ __launch_bounds__(256) void k_dn_bn_bwd_apply(const DnBnP p) {
    __shared__ float sp[7][DN_CMAX];
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ da = reinterpret_cast<const T*>(p.da);
    float* __restrict__ G = p.G;
    const int t = threadIdx.x, C = p.C, cg = C >> 3;
    const float inv_m = 1.0f / (float)p.M;
    for (int c = t; c < C; c += 256) {
        const float mean = p.batch ? p.tab[c] : p.running_mean[c];
        const float is = p.batch ? p.tab[2 * (size_t)p.ldt + c] : dn_running_invstd(p.running_var[c], p.eps);
        const float ga = p.gamma[c];
        sp[0][c] = mean; sp[1][c] = is; sp[2][c] = ga; sp[3][c] = p.beta[c];
        sp[4][c] = ga * is;
        sp[5][c] = p.batch ? p.sums[c] * inv_m : 0.f;
        sp[6][c] = p.batch ? p.sums[C + c] * inv_m : 0.f;
    }
    __syncthreads();
    const long long m0 = (long long)blockIdx.x * p.rows_pb;
    const int rows = (int)((m0 + p.rows_pb < p.M ? m0 + p.rows_pb : p.M) - m0);
    const int items = rows * cg;
    for (int j = t; j < items; j += 256) {
        const int r = j / cg, c = (j - r * cg) << 3;
        const long long m = m0 + r;
        float xv[8], gv[8], o[8];
        load8<T>(x, (size_t)m * p.ldx + c, xv);
        load8<T>(da, (size_t)m * C + c, gv);
        const size_t go = (size_t)m * p.ldg + c;
        if (p.accumulate) load8<float>(G, go, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float mean = sp[0][c + e], is = sp[1][c + e];
            const float xh = (xv[e] - mean) * is;
            float g = gv[e];
            if (RELU) g = dn_relu_on<T>(dn_affine(xv[e], mean, is, sp[2][c + e], sp[3][c + e])) ? g : 0.f;
            const float d = sp[4][c + e] * (g - sp[5][c + e] - xh * sp[6][c + e]);
            o[e] = p.accumulate ? o[e] + d : d;
        }
        store8<float>(G, go, o);
    }
}

// dst[m][cd + .] = src[m][cs + .] for C channels, 8 per thread
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void k_dn_copy(const TS* __restrict__ src, long long lds, int cs, TD* __restrict__ dst,
                                                 long long ldd, int cd, long long M, int C) {
    const int cg = C >> 3;
    const long long total = M * cg;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long m = i / cg;
        const int c = (int)(i - m * cg) << 3;
        float v[8];
        load8<TS>(src, (size_t)m * lds + cs + c, v);
        store8<TD>(dst, (size_t)m * ldd + cd + c, v);
    }
}

// nn.AvgPool2d(2, 2) on NHWC, H and W even
template <typename T>
__global__ __launch_bounds__(256) void k_avgpool_fwd(const T* __restrict__ x, T* __restrict__ y, long long total, int Ho, int Wo,
                                                     int C) {
    const int cg = C >> 3;
    const size_t rowx = (size_t)2 * Wo * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % cg) << 3;
        long long r = i / cg;
        const int wo = (int)(r % Wo);
        r /= Wo;                                              // = n * Ho + ho; the input row pair starts at 2 * r
        const size_t e = ((size_t)r * 2 * (2 * Wo) + 2 * wo) * C + c;
        float a[8], b[8], d[8], f[8], o[8];
        load8<T>(x, e, a);
        load8<T>(x, e + C, b);
        load8<T>(x, e + rowx, d);
        load8<T>(x, e + rowx + C, f);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = ((a[k] + b[k]) + (d[k] + f[k])) * 0.25f;
        store8<T>(y, (size_t)i * 8, o);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_avgpool_bwd(const T* __restrict__ dy, T* __restrict__ dx, long long total, int H, int W,
                                                     int C) {
    const int cg = C >> 3, Wo = W >> 1, Ho = H >> 1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % cg) << 3;
        long long r = i / cg;
        const int w = (int)(r % W);
        r /= W;
        const int h = (int)(r % H);
        const long long n = r / H;
        float g[8];
        load8<T>(dy, (((size_t)n * Ho + (h >> 1)) * Wo + (w >> 1)) * C + c, g);
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] *= 0.25f;
        store8<T>(dx, (size_t)i * 8, g);
    }
}

unsigned dn_grid(long long total) {
    const long long b = cr_cdiv(total, 256);
    return (unsigned)(b < 8192 ? b : 8192);
}

bool dn_slice_ok(int64_t M, int64_t ld, int c0, int C) {
    return M > 0 && C >= 32 && C <= DN_CMAX && C % 32 == 0 && c0 >= 0 && c0 % 8 == 0 && ld % 8 == 0 && (int64_t)c0 + C <= ld;
}

// rows per workgroup of the two apply kernels: about 1024 8-channel items each
int dn_rows_per_block(int C) {
    const int r = 1024 / (C >> 3);
    return r < 1 ? 1 : r;
}

}  // namespace

extern "C" int cr_dense_stats(cr_ctx* ctx, const void* x, int64_t M, int64_t ld, int c0, int C, float* tab, int ldt, int tab_off,
                              float eps, float* ws, int act_f32) {
    CR_CHECK_ARG(ctx && x && tab && ws, "cr_dense_stats: NULL pointer");
    CR_CHECK_ARG(dn_slice_ok(M, ld, c0, C), "cr_dense_stats: bad slice M=%lld ld=%lld c0=%d C=%d (C %% 32 == 0, 32..1024)",
                 (long long)M, (long long)ld, c0, C);
    CR_CHECK_ARG(tab_off >= 0 && (int64_t)tab_off + C <= ldt, "cr_dense_stats: table range %d + %d exceeds %d", tab_off, C, ldt);
    DnPartP p = {};
    p.x = x; p.part = ws; p.M = M; p.ldx = ld; p.C = C; p.c0 = c0; p.rows_pp = (int)dn_rows_per_part(M);
    const int nparts = (int)cr_cdiv(M, p.rows_pp);
    const dim3 grid((unsigned)nparts, (unsigned)(C / 32));
    if (act_f32) hipLaunchKernelGGL((k_dn_partial<float, 0>), grid, dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL((k_dn_partial<u16, 0>), grid, dim3(256), 0, ctx->stream, p);
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dn_final<0>, dim3((unsigned)(C / 32)), dim3(256), 0, ctx->stream, ws, nparts, C, (double)M, eps, tab, ldt,
                       tab_off, (float*)nullptr, (float*)nullptr, (float*)nullptr);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dense_stats_finalize(cr_ctx* ctx, const float* stats, int nparts, int C, int64_t M, float* tab, int ldt,
                                       int tab_off, float eps) {
    CR_CHECK_ARG(ctx && stats && tab, "cr_dense_stats_finalize: NULL pointer");
    CR_CHECK_ARG(M > 0 && nparts > 0 && C >= 32 && C <= DN_CMAX && C % 32 == 0, "cr_dense_stats_finalize: bad dims M=%lld nparts=%d C=%d",
                 (long long)M, nparts, C);
    CR_CHECK_ARG(tab_off >= 0 && (int64_t)tab_off + C <= ldt, "cr_dense_stats_finalize: table range %d + %d exceeds %d", tab_off, C,
                 ldt);
    hipLaunchKernelGGL(k_dn_final<0>, dim3((unsigned)(C / 32)), dim3(256), 0, ctx->stream, stats, nparts, C, (double)M, eps, tab,
                       ldt, tab_off, (float*)nullptr, (float*)nullptr, (float*)nullptr);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dense_slice_store(cr_ctx* ctx, const void* src, void* x, int64_t M, int64_t ld, int c0, int C, int act_f32) {
    CR_CHECK_ARG(ctx && src && x, "cr_dense_slice_store: NULL pointer");
    CR_CHECK_ARG(M > 0 && C >= 8 && C % 8 == 0 && c0 >= 0 && c0 % 8 == 0 && ld % 8 == 0 && (int64_t)c0 + C <= ld,
                 "cr_dense_slice_store: bad slice M=%lld ld=%lld c0=%d C=%d", (long long)M, (long long)ld, c0, C);
    const unsigned grid = dn_grid(M * (C >> 3));
    if (act_f32)
        hipLaunchKernelGGL((k_dn_copy<float, float>), dim3(grid), dim3(256), 0, ctx->stream, (const float*)src, (long long)C, 0,
                           (float*)x, (long long)ld, c0, (long long)M, C);
    else
        hipLaunchKernelGGL((k_dn_copy<u16, u16>), dim3(grid), dim3(256), 0, ctx->stream, (const u16*)src, (long long)C, 0, (u16*)x,
                           (long long)ld, c0, (long long)M, C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dense_slice_gather(cr_ctx* ctx, const float* g, int64_t M, int64_t ld, int c0, int C, void* dst, int act_f32) {
    CR_CHECK_ARG(ctx && g && dst, "cr_dense_slice_gather: NULL pointer");
    CR_CHECK_ARG(M > 0 && C >= 8 && C % 8 == 0 && c0 >= 0 && c0 % 8 == 0 && ld % 8 == 0 && (int64_t)c0 + C <= ld,
                 "cr_dense_slice_gather: bad slice M=%lld ld=%lld c0=%d C=%d", (long long)M, (long long)ld, c0, C);
    const unsigned grid = dn_grid(M * (C >> 3));
    if (act_f32)
        hipLaunchKernelGGL((k_dn_copy<float, float>), dim3(grid), dim3(256), 0, ctx->stream, g, (long long)ld, c0, (float*)dst,
                           (long long)C, 0, (long long)M, C);
    else
        hipLaunchKernelGGL((k_dn_copy<float, u16>), dim3(grid), dim3(256), 0, ctx->stream, g, (long long)ld, c0, (u16*)dst,
                           (long long)C, 0, (long long)M, C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dense_bn_fwd(cr_ctx* ctx, const void* x, int64_t M, int64_t ld, int C, const float* tab, int ldt,
                               const float* gamma, const float* beta, float* running_mean, float* running_var, float eps,
                               float momentum, int batch_stats, int relu, void* out, int act_f32) {
    CR_CHECK_ARG(ctx && x && gamma && beta && out, "cr_dense_bn_fwd: NULL pointer");
    CR_CHECK_ARG(dn_slice_ok(M, ld, 0, C), "cr_dense_bn_fwd: bad slice M=%lld ld=%lld C=%d (C %% 32 == 0, 32..1024)", (long long)M,
                 (long long)ld, C);
    if (batch_stats) CR_CHECK_ARG(tab && ldt >= C && (running_mean != nullptr) == (running_var != nullptr),
                                  "cr_dense_bn_fwd: batch statistics need the table (ldt %d >= C %d)", ldt, C);
    else CR_CHECK_ARG(running_mean && running_var, "cr_dense_bn_fwd: running statistics mode without running statistics");
    DnBnP p = {};
    p.x = x; p.out = out; p.tab = tab; p.ldt = ldt; p.gamma = gamma; p.beta = beta; p.running_mean = running_mean;
    p.running_var = running_var; p.M = M; p.ldx = ld; p.C = C; p.relu = relu; p.batch = batch_stats ? 1 : 0;
    p.rows_pb = dn_rows_per_block(C); p.eps = eps; p.momentum = momentum;
    const dim3 grid((unsigned)cr_cdiv(M, p.rows_pb));
    if (act_f32) hipLaunchKernelGGL(k_dn_bn_fwd<float>, grid, dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL(k_dn_bn_fwd<u16>, grid, dim3(256), 0, ctx->stream, p);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dense_bn_bwd(cr_ctx* ctx, const void* da, const void* x, int64_t M, int64_t ld, int C, const float* tab, int ldt,
                               const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                               float eps, int batch_stats, int relu, float* g, int64_t ldg, int accumulate, float* dgamma,
                               float* dbeta, float* ws, int act_f32) {
    CR_CHECK_ARG(ctx && da && x && gamma && beta && g && dgamma && dbeta && ws, "cr_dense_bn_bwd: NULL pointer");
    CR_CHECK_ARG(dn_slice_ok(M, ld, 0, C) && ldg >= C && ldg % 8 == 0,
                 "cr_dense_bn_bwd: bad slice M=%lld ld=%lld ldg=%lld C=%d (C %% 32 == 0, 32..1024)", (long long)M, (long long)ld,
                 (long long)ldg, C);
    if (batch_stats) CR_CHECK_ARG(tab && ldt >= C, "cr_dense_bn_bwd: batch statistics need the table (ldt %d >= C %d)", ldt, C);
    else CR_CHECK_ARG(running_mean && running_var, "cr_dense_bn_bwd: running statistics mode without running statistics");
    DnPartP q = {};
    q.x = x; q.da = da; q.gamma = gamma; q.beta = beta; q.part = ws; q.M = M; q.ldx = ld; q.C = C; q.c0 = 0;
    q.running = batch_stats ? 0 : 1; q.eps = eps; q.rows_pp = (int)dn_rows_per_part(M);
    q.mean = batch_stats ? tab : running_mean;
    q.invstd = batch_stats ? tab + 2 * (size_t)ldt : running_var;
    const int nparts = (int)cr_cdiv(M, q.rows_pp);
    float* sums = ws + (size_t)nparts * 2 * C;
    const dim3 pgrid((unsigned)nparts, (unsigned)(C / 32));
    if (act_f32 && relu) hipLaunchKernelGGL((k_dn_partial<float, 2>), pgrid, dim3(256), 0, ctx->stream, q);
    else if (act_f32) hipLaunchKernelGGL((k_dn_partial<float, 1>), pgrid, dim3(256), 0, ctx->stream, q);
    else if (relu) hipLaunchKernelGGL((k_dn_partial<u16, 2>), pgrid, dim3(256), 0, ctx->stream, q);
    else hipLaunchKernelGGL((k_dn_partial<u16, 1>), pgrid, dim3(256), 0, ctx->stream, q);
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dn_final<1>, dim3((unsigned)(C / 32)), dim3(256), 0, ctx->stream, ws, nparts, C, (double)M, eps,
                       (float*)nullptr, 0, 0, sums, dgamma, dbeta);
    CR_LAUNCH_CHECK();
    DnBnP p = {};
    p.x = x; p.da = da; p.G = g; p.tab = tab; p.ldt = ldt; p.gamma = gamma; p.beta = beta;
    p.running_mean = const_cast<float*>(running_mean); p.running_var = const_cast<float*>(running_var); p.sums = sums;
    p.M = M; p.ldx = ld; p.ldg = ldg; p.C = C; p.relu = relu; p.batch = batch_stats ? 1 : 0; p.accumulate = accumulate;
    p.rows_pb = dn_rows_per_block(C); p.eps = eps;
    const dim3 grid((unsigned)cr_cdiv(M, p.rows_pb));
    if (act_f32 && relu) hipLaunchKernelGGL((k_dn_bn_bwd_apply<float, true>), grid, dim3(256), 0, ctx->stream, p);
    else if (act_f32) hipLaunchKernelGGL((k_dn_bn_bwd_apply<float, false>), grid, dim3(256), 0, ctx->stream, p);
    else if (relu) hipLaunchKernelGGL((k_dn_bn_bwd_apply<u16, true>), grid, dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL((k_dn_bn_bwd_apply<u16, false>), grid, dim3(256), 0, ctx->stream, p);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_avgpool2x2_fwd(cr_ctx* ctx, const void* x, void* y, int N, int H, int W, int C, int act_f32) {
    CR_CHECK_ARG(ctx && x && y, "cr_avgpool2x2_fwd: NULL pointer");
    CR_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % 8 == 0,
                 "cr_avgpool2x2_fwd: needs even H, W and C %% 8 == 0 (N=%d H=%d W=%d C=%d)", N, H, W, C);
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 8);
    if (act_f32)
        hipLaunchKernelGGL(k_avgpool_fwd<float>, dim3(dn_grid(total)), dim3(256), 0, ctx->stream, (const float*)x, (float*)y, total,
                           H / 2, W / 2, C);
    else
        hipLaunchKernelGGL(k_avgpool_fwd<u16>, dim3(dn_grid(total)), dim3(256), 0, ctx->stream, (const u16*)x, (u16*)y, total, H / 2,
                           W / 2, C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_avgpool2x2_bwd(cr_ctx* ctx, const void* dy, void* dx, int N, int H, int W, int C, int act_f32) {
    CR_CHECK_ARG(ctx && dy && dx, "cr_avgpool2x2_bwd: NULL pointer");
    CR_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % 8 == 0,
                 "cr_avgpool2x2_bwd: needs even H, W and C %% 8 == 0 (N=%d H=%d W=%d C=%d)", N, H, W, C);
    const long long total = (long long)N * H * W * (C / 8);
    if (act_f32)
        hipLaunchKernelGGL(k_avgpool_bwd<float>, dim3(dn_grid(total)), dim3(256), 0, ctx->stream, (const float*)dy, (float*)dx, total,
                           H, W, C);
    else
        hipLaunchKernelGGL(k_avgpool_bwd<u16>, dim3(dn_grid(total)), dim3(256), 0, ctx->stream, (const u16*)dy, (u16*)dx, total, H, W,
                           C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}
