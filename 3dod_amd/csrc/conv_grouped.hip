// Grouped 3x3 convolution (pad 1, stride 1 or 2, Cin == Cout, groups in {32, 64}, 2..32 channels per group): the middle
// convolution of DLA's BottleneckX blocks (cubercnn/modeling/backbone/dla.py:112-153 of the reference).
//
// Per group the contraction is 9 * cg = 18..288 long and the layers are memory-bound, so all three directions are direct
// convolutions on the vector ALU (f32 FMA, f32 accumulation for f32 and bf16 activations alike), in plain C++:
//   * activations NHWC, weights f32 KRSC (Cout, 3, 3, cg) -- the backward-data pass reads the same array, no transposed copy;
//   * a workgroup covers 64 consecutive channels (lanes = channels: stores and the dy reads of the weight gradient are
//     256-byte rows) of 64 pixels; a thread keeps one tap's cg weights in registers for 4 pixels at a time and reads the cg
//     input channels of its group with 16-byte loads where cg allows;
//   * every halo access is predicated, element offsets are 64-bit, grids follow from the problem size alone;
//   * the forward pass can emit BatchNorm statistics rows in cr_bn_fwd's layout (one row per 64 output pixels = one
//     workgroup row, summed in a fixed order);
//   * the weight gradient uses no atomics: workgroup (s, cb) writes the partial sums of pixel range s into the caller's
//     workspace and a second kernel adds the ranges in index order -> bit-identical from run to run.
#include "cr_common.h"
#include "cr_elem.h"

namespace {

// V consecutive channels at element index e (a multiple of V) as floats
template <typename T, int V> __device__ __forceinline__ void ldv(const T* __restrict__ p, size_t e, float* f) {
    if constexpr (V == 2) {
        if constexpr (sizeof(T) == 4) {
            const float2 a = *reinterpret_cast<const float2*>(p + e);
            f[0] = a.x; f[1] = a.y;
        } else {
            const unsigned v = *reinterpret_cast<const unsigned*>(p + e);
            f[0] = bf2f((u16)(v & 0xffff)); f[1] = bf2f((u16)(v >> 16));
        }
    } else if constexpr (V == 4) {
        load4<T>(p, e, f);
    } else {
#pragma unroll
        for (int i = 0; i < V; i += 8) load8<T>(p, e + i, f + i);
    }
}

template <typename T> __device__ __forceinline__ float as_stored(float v) {
    if constexpr (sizeof(T) == 4) return v; else return bf2f(f2bf(v));
}
template <typename T> __device__ __forceinline__ void st1(T* __restrict__ p, size_t e, float v) {
    if constexpr (sizeof(T) == 4) p[e] = v; else p[e] = f2bf(v);
}

struct GConvP {
    const void* x;       // forward: input; backward-data: dy; weight gradient: x
    const void* dy;      // weight gradient only
    const float* w;      // (C, 3, 3, cg)
    void* y;             // forward: output; backward-data: dx
    const float* bias;
    const void* res;     // forward: residual; backward-data: accumulate
    float* stats;
    int relu;
    int N, H, W, Ho, Wo, C;
    long long M;         // pixels the grid runs over
};

constexpr int PXB = 64;          // pixels per workgroup (= one statistics row)
constexpr int PXT = 16;          // pixels per thread, in batches of 4

// ---------------------------------------------------------------------------------------------------------------------
// forward: thread (cx, py) = output channel blockIdx.y * 64 + cx, output pixels blockIdx.x * 64 + py * 16 .. + 15
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int CG, int STRIDE>
__global__ __launch_bounds__(256) void k_gconv_fwd(const GConvP p) {
    __shared__ float sS[4][2][64];
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ res = reinterpret_cast<const T*>(p.res);
    T* __restrict__ y = reinterpret_cast<T*>(p.y);
    const int cx = threadIdx.x, py = threadIdx.y;
    const int co = blockIdx.y * 64 + cx;
    const int gbase = (co / CG) * CG;
    const float* __restrict__ wrow = p.w + (size_t)co * 9 * CG;
    const long long p0 = (long long)blockIdx.x * PXB + py * PXT;
    const float bias = p.bias ? p.bias[co] : 0.f;
    float ssum = 0.f, ssq = 0.f;
    for (int b = 0; b < PXT; b += 4) {
        int n[4], ho[4], wo[4];
        bool ok[4];
        float acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long q = p0 + b + j;
            ok[j] = q < p.M;
            const long long qq = ok[j] ? q : 0;
            wo[j] = (int)(qq % p.Wo);
            const long long t = qq / p.Wo;
            ho[j] = (int)(t % p.Ho);
            n[j] = (int)(t / p.Ho);
            acc[j] = 0.f;
        }
        if (!ok[0]) break;                                   // pixels are ascending: the rest of this thread is past the end
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            float wv[CG];
            ldv<float, CG>(wrow, (size_t)tap * CG, wv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int hi = ho[j] * STRIDE + r - 1, wi = wo[j] * STRIDE + s - 1;
                if (ok[j] && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
                    float xv[CG];
                    ldv<T, CG>(x, (((size_t)n[j] * p.H + hi) * p.W + wi) * p.C + gbase, xv);
#pragma unroll
                    for (int i = 0; i < CG; ++i) acc[j] = fmaf(xv[i], wv[i], acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!ok[j]) continue;
            const size_t o = (size_t)(p0 + b + j) * p.C + co;
            float v = acc[j] + bias;
            const float vs = as_stored<T>(v);                // statistics are those of the values BatchNorm will read
            ssum += vs;
            ssq = fmaf(vs, vs, ssq);
            if (res) v += load1<T>(res, o);
            if (p.relu) v = fmaxf(v, 0.f);
            st1<T>(y, o, v);
        }
    }
    if (p.stats == nullptr) return;                          // block-uniform
    sS[py][0][cx] = ssum;
    sS[py][1][cx] = ssq;
    __syncthreads();
    if (py < 2) {
        const float a = ((sS[0][py][cx] + sS[1][py][cx]) + sS[2][py][cx]) + sS[3][py][cx];      // fixed order
        p.stats[((size_t)blockIdx.x * 2 + py) * p.C + co] = a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward-data: thread (cx, py) = input channel blockIdx.y * 64 + cx, input pixels blockIdx.x * 64 + py * 16 .. + 15;
// dx[n,h,w,g*cg+ci] = sum over taps (r,s) with ho * stride + r - 1 == h (same for w) and co of dy[n,ho,wo,g*cg+co] *
// w[g*cg+co][r][s][ci]  (+ accumulate)
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int CG, int STRIDE>
__global__ __launch_bounds__(256) void k_gconv_bwd_data(const GConvP p) {
    const T* __restrict__ dy = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ acc_in = reinterpret_cast<const T*>(p.res);
    T* __restrict__ dx = reinterpret_cast<T*>(p.y);
    const int cx = threadIdx.x, py = threadIdx.y;
    const int c = blockIdx.y * 64 + cx;
    const int gbase = (c / CG) * CG, ci = c - gbase;
    const float* __restrict__ wg = p.w + (size_t)gbase * 9 * CG + ci;
    const long long p0 = (long long)blockIdx.x * PXB + py * PXT;
    for (int b = 0; b < PXT; b += 4) {
        int n[4], h[4], wq[4];
        bool ok[4];
        float acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long q = p0 + b + j;
            ok[j] = q < p.M;
            const long long qq = ok[j] ? q : 0;
            wq[j] = (int)(qq % p.W);
            const long long t = qq / p.W;
            h[j] = (int)(t % p.H);
            n[j] = (int)(t / p.H);
            acc[j] = 0.f;
        }
        if (!ok[0]) break;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            float wv[CG];
#pragma unroll
            for (int o = 0; o < CG; ++o) wv[o] = wg[(size_t)o * 9 * CG + tap * CG];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int th = h[j] + 1 - r, tw = wq[j] + 1 - s;
                bool in = ok[j] && th >= 0 && tw >= 0;
                int ho = th, wo = tw;
                if (STRIDE == 2) {
                    in = in && ((th & 1) == 0) && ((tw & 1) == 0);
                    ho = th >> 1;
                    wo = tw >> 1;
                }
                if (in && ho < p.Ho && wo < p.Wo) {
                    float gv[CG];
                    ldv<T, CG>(dy, (((size_t)n[j] * p.Ho + ho) * p.Wo + wo) * p.C + gbase, gv);
#pragma unroll
                    for (int o = 0; o < CG; ++o) acc[j] = fmaf(gv[o], wv[o], acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!ok[j]) continue;
            const size_t o = (size_t)(p0 + b + j) * p.C + c;
            float v = acc[j];
            if (acc_in) v += load1<T>(acc_in, o);
            st1<T>(dx, o, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient, pass 1: workgroup (split, cb), thread (cx, tap): partial dw[co][tap][0..cg) over output pixels
// [split * range, (split + 1) * range) into part[split][C * 9 * cg]; the tap-0 threads also sum dy (bias gradient) into
// bpart[split][C].  Pass 2 adds the splits in index order.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int CG, int STRIDE>
__global__ __launch_bounds__(576) void k_gconv_wgrad(const GConvP p, long long range, float* __restrict__ part,
                                                     float* __restrict__ bpart) {
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ dy = reinterpret_cast<const T*>(p.dy);
    const int cx = threadIdx.x, tap = threadIdx.y;
    const int r = tap / 3, s = tap - r * 3;
    const int co = blockIdx.y * 64 + cx;
    const int gbase = (co / CG) * CG;
    const long long q0 = (long long)blockIdx.x * range;
    const long long q1 = (q0 + range < p.M) ? q0 + range : p.M;
    int wo = (int)(q0 % p.Wo);
    long long t = q0 / p.Wo;
    int ho = (int)(t % p.Ho);
    int n = (int)(t / p.Ho);
    float acc[CG];
#pragma unroll
    for (int i = 0; i < CG; ++i) acc[i] = 0.f;
    float bsum = 0.f;
    for (long long q = q0; q < q1; ++q) {
        const float g = load1<T>(dy, (size_t)q * p.C + co);
        bsum += g;
        const int hi = ho * STRIDE + r - 1, wi = wo * STRIDE + s - 1;
        if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
            float xv[CG];
            ldv<T, CG>(x, (((size_t)n * p.H + hi) * p.W + wi) * p.C + gbase, xv);
#pragma unroll
            for (int i = 0; i < CG; ++i) acc[i] = fmaf(g, xv[i], acc[i]);
        }
        if (++wo == p.Wo) {
            wo = 0;
            if (++ho == p.Ho) { ho = 0; ++n; }
        }
    }
    const size_t E = (size_t)p.C * 9 * CG;
    float* dst = part + (size_t)blockIdx.x * E + ((size_t)co * 9 + tap) * CG;
    if constexpr (CG == 2) {
        *reinterpret_cast<float2*>(dst) = make_float2(acc[0], acc[1]);
    } else {
#pragma unroll
        for (int i = 0; i < CG; i += 4) *reinterpret_cast<float4*>(dst + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
    }
    if (tap == 0) bpart[(size_t)blockIdx.x * p.C + co] = bsum;
}

// pass 2: dw[e] = (accumulate ? dw[e] : 0) + sum_s part[s][e] for e < E; dbias[c] += sum_s bpart[s][c] (when given)
__global__ __launch_bounds__(256) void k_gconv_wgrad_reduce(const float* __restrict__ part, const float* __restrict__ bpart,
                                                            int nsplit, long long E, int C, float* __restrict__ dw,
                                                            float* __restrict__ dbias, int accumulate) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < E) {
        float a = 0.f;
        for (int sp = 0; sp < nsplit; ++sp) a += part[(size_t)sp * E + e];
        dw[e] = accumulate ? dw[e] + a : a;
    } else if (e < E + C && dbias != nullptr) {
        const int c = (int)(e - E);
        float a = 0.f;
        for (int sp = 0; sp < nsplit; ++sp) a += bpart[(size_t)sp * C + c];
        dbias[c] += a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
int check_geometry(const char* who, int N, int H, int W, int Cin, int Cout, int groups, int ks, int stride, int pad,
                   int act_f32, int* cg) {
    CR_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "%s: N, H, W must be >= 1 (got %d, %d, %d)", who, N, H, W);
    CR_CHECK_ARG(ks == 3 && pad == 1, "%s: only ks = 3, pad = 1 (got ks %d, pad %d)", who, ks, pad);
    CR_CHECK_ARG(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (got %d)", who, stride);
    CR_CHECK_ARG(Cin == Cout, "%s: Cin must equal Cout (got %d, %d)", who, Cin, Cout);
    CR_CHECK_ARG(groups == 32 || groups == 64, "%s: groups must be 32 or 64 (got %d)", who, groups);
    CR_CHECK_ARG(Cin > 0 && Cin % groups == 0, "%s: channels (%d) must be a positive multiple of groups (%d)", who, Cin, groups);
    const int g = Cin / groups;
    CR_CHECK_ARG(g == 2 || g == 4 || g == 8 || g == 16 || g == 32,
                 "%s: channels per group must be 2, 4, 8, 16 or 32 (got %d = %d / %d)", who, g, Cin, groups);
    CR_CHECK_ARG(act_f32 >= 0 && act_f32 <= 2, "%s: act_f32 must be 0, 1 or 2 (got %d)", who, act_f32);
    *cg = g;
    return CR_OK;
}

enum { FWD = 0, BWD_DATA = 1 };

template <int DIR, typename T, int CG>
void launch_dir_s(cr_ctx* ctx, const GConvP& p, int stride, dim3 grid) {
    const dim3 block(64, 4);
    if (DIR == FWD) {
        if (stride == 1) hipLaunchKernelGGL((k_gconv_fwd<T, CG, 1>), grid, block, 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_gconv_fwd<T, CG, 2>), grid, block, 0, ctx->stream, p);
    } else {
        if (stride == 1) hipLaunchKernelGGL((k_gconv_bwd_data<T, CG, 1>), grid, block, 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_gconv_bwd_data<T, CG, 2>), grid, block, 0, ctx->stream, p);
    }
}

template <int DIR, typename T>
void launch_dir(cr_ctx* ctx, const GConvP& p, int cg, int stride) {
    const dim3 grid((unsigned)cr_cdiv(p.M, PXB), (unsigned)(p.C / 64));
    switch (cg) {
        case 2: launch_dir_s<DIR, T, 2>(ctx, p, stride, grid); break;
        case 4: launch_dir_s<DIR, T, 4>(ctx, p, stride, grid); break;
        case 8: launch_dir_s<DIR, T, 8>(ctx, p, stride, grid); break;
        case 16: launch_dir_s<DIR, T, 16>(ctx, p, stride, grid); break;
        default: launch_dir_s<DIR, T, 32>(ctx, p, stride, grid); break;
    }
}

template <typename T, int CG>
void launch_wgrad_s(cr_ctx* ctx, const GConvP& p, int stride, dim3 grid, long long range, float* part, float* bpart) {
    const dim3 block(64, 9);
    if (stride == 1) hipLaunchKernelGGL((k_gconv_wgrad<T, CG, 1>), grid, block, 0, ctx->stream, p, range, part, bpart);
    else hipLaunchKernelGGL((k_gconv_wgrad<T, CG, 2>), grid, block, 0, ctx->stream, p, range, part, bpart);
}

template <typename T>
void launch_wgrad(cr_ctx* ctx, const GConvP& p, int cg, int stride, dim3 grid, long long range, float* part, float* bpart) {
    switch (cg) {
        case 2: launch_wgrad_s<T, 2>(ctx, p, stride, grid, range, part, bpart); break;
        case 4: launch_wgrad_s<T, 4>(ctx, p, stride, grid, range, part, bpart); break;
        case 8: launch_wgrad_s<T, 8>(ctx, p, stride, grid, range, part, bpart); break;
        case 16: launch_wgrad_s<T, 16>(ctx, p, stride, grid, range, part, bpart); break;
        default: launch_wgrad_s<T, 32>(ctx, p, stride, grid, range, part, bpart); break;
    }
}

}  // namespace

extern "C" int cr_conv2d_grouped_fwd(cr_ctx* ctx, const void* x, const float* w, void* y, int N, int H, int W, int Cin,
                                     int Cout, int groups, int ks, int stride, int pad, const float* bias,
                                     const void* residual, int relu, float* stats, int act_f32) {
    CR_CHECK_ARG(ctx && x && w && y, "cr_conv2d_grouped_fwd: NULL pointer");
    int cg = 0;
    if (int rc = check_geometry("cr_conv2d_grouped_fwd", N, H, W, Cin, Cout, groups, ks, stride, pad, act_f32, &cg)) return rc;
    GConvP p = {};
    p.x = x; p.w = w; p.y = y; p.bias = bias; p.res = residual; p.stats = stats; p.relu = relu;
    p.N = N; p.H = H; p.W = W; p.C = Cin;
    p.Ho = (H + 2 - 3) / stride + 1;
    p.Wo = (W + 2 - 3) / stride + 1;
    p.M = (long long)N * p.Ho * p.Wo;
    CR_CHECK_ARG(cr_cdiv(p.M, PXB) <= 0x7fffffffLL, "cr_conv2d_grouped_fwd: too many output pixels (%lld)", p.M);
    if (act_f32) launch_dir<FWD, float>(ctx, p, cg, stride);
    else launch_dir<FWD, u16>(ctx, p, cg, stride);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_conv2d_grouped_bwd_data(cr_ctx* ctx, const void* dy, const float* w, void* dx, int N, int H, int W,
                                          int Cin, int Cout, int groups, int ks, int stride, int pad, int act_f32,
                                          const void* accumulate) {
    CR_CHECK_ARG(ctx && dy && w && dx, "cr_conv2d_grouped_bwd_data: NULL pointer");
    int cg = 0;
    if (int rc = check_geometry("cr_conv2d_grouped_bwd_data", N, H, W, Cin, Cout, groups, ks, stride, pad, act_f32, &cg)) return rc;
    GConvP p = {};
    p.x = dy; p.w = w; p.y = dx; p.res = accumulate;
    p.N = N; p.H = H; p.W = W; p.C = Cin;
    p.Ho = (H + 2 - 3) / stride + 1;
    p.Wo = (W + 2 - 3) / stride + 1;
    p.M = (long long)N * H * W;
    CR_CHECK_ARG(cr_cdiv(p.M, PXB) <= 0x7fffffffLL, "cr_conv2d_grouped_bwd_data: too many input pixels (%lld)", p.M);
    if (act_f32) launch_dir<BWD_DATA, float>(ctx, p, cg, stride);
    else launch_dir<BWD_DATA, u16>(ctx, p, cg, stride);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_conv2d_grouped_bwd_weight(cr_ctx* ctx, const void* dy, const void* x, float* dw, float* dbias, int N,
                                            int H, int W, int Cin, int Cout, int groups, int ks, int stride, int pad,
                                            int accumulate, int act_f32, float* ws, int64_t ws_floats) {
    CR_CHECK_ARG(ctx && dy && x && dw && ws, "cr_conv2d_grouped_bwd_weight: NULL pointer");
    int cg = 0;
    if (int rc = check_geometry("cr_conv2d_grouped_bwd_weight", N, H, W, Cin, Cout, groups, ks, stride, pad, act_f32, &cg)) return rc;
    GConvP p = {};
    p.x = x; p.dy = dy;
    p.N = N; p.H = H; p.W = W; p.C = Cin;
    p.Ho = (H + 2 - 3) / stride + 1;
    p.Wo = (W + 2 - 3) / stride + 1;
    p.M = (long long)N * p.Ho * p.Wo;
    // pixel ranges of at least 128 output pixels, at most 256 of them: a function of the problem alone
    const long long range = cr_cdiv(p.M, 256) > 128 ? cr_cdiv(p.M, 256) : 128;
    const int nsplit = (int)cr_cdiv(p.M, range);
    const long long E = (long long)Cin * 9 * cg;
    CR_CHECK_ARG(ws_floats >= (int64_t)nsplit * (E + Cin),
                 "cr_conv2d_grouped_bwd_weight: workspace of %lld floats, %lld needed (splits * (Cout * 9 * cg + Cout), splits = %d)",
                 (long long)ws_floats, (long long)nsplit * (E + Cin), nsplit);
    float* part = ws;
    float* bpart = ws + (size_t)nsplit * E;
    const dim3 grid((unsigned)nsplit, (unsigned)(Cin / 64));
    if (act_f32) launch_wgrad<float>(ctx, p, cg, stride, grid, range, part, bpart);
    else launch_wgrad<u16>(ctx, p, cg, stride, grid, range, part, bpart);
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gconv_wgrad_reduce, dim3((unsigned)cr_cdiv(E + Cin, 256)), dim3(256), 0, ctx->stream, part, bpart,
                       nsplit, E, Cin, dw, dbias, accumulate);
    CR_LAUNCH_CHECK();
    return CR_OK;
}
