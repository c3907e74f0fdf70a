// ShuffleNetV2 trunk kernels (cubercnn/modeling/backbone/shufflenet.py of the reference takes torchvision's
// shufflenet_v2_x1_0): everything here is memory-bound vector-ALU work in plain C++.
//
//   * depthwise 3x3 convolution (pad 1, stride 1 or 2), NHWC activations in f32 or bf16, f32 weights (C, 3, 3) in every
//     precision mode, f32 accumulation, C % 8 == 0.  A thread owns 8 consecutive channels (16-byte loads for bf16, two for
//     f32; consecutive lanes = consecutive channel groups) and 4 consecutive pixels; its nine taps' weights (72 floats) stay
//     in registers.  Halo accesses are predicated, element offsets are 64-bit, grids follow from the problem size alone.
//     The forward pass can emit BatchNorm statistics rows in cr_bn_fwd's layout (one row per 64 output pixels, summed in a
//     fixed order).  The weight gradient uses no atomics: a workgroup writes the partial sums of its pixel range into the
//     caller's workspace and a second kernel adds the ranges in index order -> bit-identical from run to run.
//   * the unit tail: channel concatenation + channel_shuffle(groups = 2) as ONE pass with 16-byte stores, and its backward
//     (de-interleave).  A two-half tensor of 2 * bf logical channels is stored as [half 0 | pad | half 1 | pad] with each
//     half padded to wp channels; pads are written as zero.
//   * pack / unpack between logical parameters and their zero-padded compute copies, any number of tensors per launch.
#include "cr_common.h"
#include "cr_elem.h"

namespace {

template <typename T> __device__ __forceinline__ float as_stored(float v) {
    if constexpr (sizeof(T) == 4) return v; else return bf2f(f2bf(v));
}

struct DwP {
    const void* x;       // forward: input; backward-data: dy; weight gradient: x
    const void* dy;      // weight gradient only
    const float* w;      // (C, 3, 3)
    void* y;             // forward: output; backward-data: dx
    const float* bias;
    const void* acc;     // backward-data: accumulate
    float* stats;
    int N, H, W, Ho, Wo, C;
    int cgb;             // channel groups (of 8) per workgroup: a power of two <= 16
    long long M;         // pixels the grid runs over
};

// the nine taps of 8 consecutive channels: w[(c0 + i) * 9 + tap] -> wv[tap][i]  (72 consecutive floats, 16-byte aligned)
__device__ __forceinline__ void load_taps(const float* __restrict__ w, int c0, float (*wv)[8]) {
    float wl[72];
    const float4* src = reinterpret_cast<const float4*>(w + (size_t)c0 * 9);
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        const float4 v = src[i];
        wl[4 * i] = v.x; wl[4 * i + 1] = v.y; wl[4 * i + 2] = v.z; wl[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[tap][i] = wl[i * 9 + tap];
}

// thread t of a 256-thread workgroup: channel group t % cgb, pixel quad (t / cgb) % 16, row t / (16 * cgb) of the
// 16 / cgb rows of 64 pixels the workgroup covers
// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int STRIDE>
__global__ __launch_bounds__(256) void k_dw_fwd(const DwP p) {
    __shared__ float sS[4096];                               // [row][quad][2][cgb * 8]
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    T* __restrict__ y = reinterpret_cast<T*>(p.y);
    const int t = threadIdx.x;
    const int cgi = t % p.cgb, quad = (t / p.cgb) & 15, row = t / (p.cgb * 16);
    const int rb = 16 / p.cgb;
    const int c0 = (blockIdx.y * p.cgb + cgi) * 8;
    const bool cok = c0 < p.C;
    const long long rowi = (long long)blockIdx.x * rb + row;
    const long long q0 = rowi * 64 + quad * 4;
    float ssum[8], ssq[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { ssum[i] = 0.f; ssq[i] = 0.f; }
    if (cok && q0 < p.M) {
        float wv[9][8], bias[8];
        load_taps(p.w, c0, wv);
#pragma unroll
        for (int i = 0; i < 8; ++i) bias[i] = p.bias ? p.bias[c0 + i] : 0.f;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const long long q = q0 + j;
            if (q >= p.M) break;
            const int wo = (int)(q % p.Wo);
            const long long tq = q / p.Wo;
            const int ho = (int)(tq % p.Ho), n = (int)(tq / p.Ho);
            float acc[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = bias[i];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int r = tap / 3, s = tap - r * 3;
                const int hi = ho * STRIDE + r - 1, wi = wo * STRIDE + s - 1;
                if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
                    float xv[8];
                    load8<T>(x, (((size_t)n * p.H + hi) * p.W + wi) * p.C + c0, xv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] = fmaf(xv[i], wv[tap][i], acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float vs = as_stored<T>(acc[i]);       // statistics are those of the values BatchNorm will read
                ssum[i] += vs;
                ssq[i] = fmaf(vs, vs, ssq[i]);
            }
            store8<T>(y, (size_t)q * p.C + c0, acc);
        }
    }
    if (p.stats == nullptr) return;                          // block-uniform
    const int cw = p.cgb * 8;
    {
        float* d0 = sS + ((size_t)((row * 16 + quad) * 2 + 0) * p.cgb + cgi) * 8;
        float* d1 = d0 + cw;
#pragma unroll
        for (int i = 0; i < 8; ++i) { d0[i] = ssum[i]; d1[i] = ssq[i]; }
    }
    __syncthreads();
    if (quad < 2 && cok && rowi * 64 < p.M) {                // quad = which (0: sum, 1: sum of squares)
        float a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = 0.f;
        for (int qd = 0; qd < 16; ++qd) {                    // fixed order
            const float* s = sS + ((size_t)((row * 16 + qd) * 2 + quad) * p.cgb + cgi) * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] += s[i];
        }
        store8<float>(p.stats, ((size_t)rowi * 2 + quad) * p.C + c0, a);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward-data: dx[n,h,w,c] = sum over taps (r,s) with ho * stride + r - 1 == h (same for w) of dy[n,ho,wo,c] * w[c][r][s]
// (+ accumulate); the grid runs over input pixels
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int STRIDE>
__global__ __launch_bounds__(256) void k_dw_bwd_data(const DwP p) {
    const T* __restrict__ dy = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ acc_in = reinterpret_cast<const T*>(p.acc);
    T* __restrict__ dx = reinterpret_cast<T*>(p.y);
    const int t = threadIdx.x;
    const int cgi = t % p.cgb, quad = (t / p.cgb) & 15, row = t / (p.cgb * 16);
    const int rb = 16 / p.cgb;
    const int c0 = (blockIdx.y * p.cgb + cgi) * 8;
    const long long q0 = ((long long)blockIdx.x * rb + row) * 64 + quad * 4;
    if (c0 >= p.C || q0 >= p.M) return;
    float wv[9][8];
    load_taps(p.w, c0, wv);
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const long long q = q0 + j;
        if (q >= p.M) break;
        const int wq = (int)(q % p.W);
        const long long tq = q / p.W;
        const int h = (int)(tq % p.H), n = (int)(tq / p.H);
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        if (acc_in) load8<T>(acc_in, (size_t)q * p.C + c0, acc);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            const int th = h + 1 - r, tw = wq + 1 - s;
            bool in = th >= 0 && tw >= 0;
            int ho = th, wo = tw;
            if (STRIDE == 2) {
                in = in && ((th & 1) == 0) && ((tw & 1) == 0);
                ho = th >> 1;
                wo = tw >> 1;
            }
            if (in && ho < p.Ho && wo < p.Wo) {
                float gv[8];
                load8<T>(dy, (((size_t)n * p.Ho + ho) * p.Wo + wo) * p.C + c0, gv);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(gv[i], wv[tap][i], acc[i]);
            }
        }
        store8<T>(dx, (size_t)q * p.C + c0, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient, pass 1: workgroup blockIdx.x owns the output pixels [split * range, (split + 1) * range); thread t =
// channel group t % cgb, slot t / cgb takes every (256 / cgb)-th pixel of the range; the slots are added in slot order
// through LDS and the workgroup writes the partial dw of its range into part[split][C * 9].  Pass 2 adds the ranges in
// index order.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, int STRIDE>
__global__ __launch_bounds__(256) void k_dw_wgrad(const DwP p, long long range, float* __restrict__ part) {
    __shared__ float sR[256 * 8];
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ dy = reinterpret_cast<const T*>(p.dy);
    const int t = threadIdx.x;
    const int cgi = t % p.cgb, slot = t / p.cgb, nslot = 256 / p.cgb;
    const int c0 = (blockIdx.y * p.cgb + cgi) * 8;
    const bool cok = c0 < p.C;
    const long long q0 = (long long)blockIdx.x * range;
    const long long q1 = (q0 + range < p.M) ? q0 + range : p.M;
    float acc[9][8];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[tap][i] = 0.f;
    if (cok) {
        for (long long q = q0 + slot; q < q1; q += nslot) {
            const int wo = (int)(q % p.Wo);
            const long long tq = q / p.Wo;
            const int ho = (int)(tq % p.Ho), n = (int)(tq / p.Ho);
            float g[8];
            load8<T>(dy, (size_t)q * p.C + c0, g);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int r = tap / 3, s = tap - r * 3;
                const int hi = ho * STRIDE + r - 1, wi = wo * STRIDE + s - 1;
                if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
                    float xv[8];
                    load8<T>(x, (((size_t)n * p.H + hi) * p.W + wi) * p.C + c0, xv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[tap][i] = fmaf(g[i], xv[i], acc[tap][i]);
                }
            }
        }
    }
    // the slots of one channel group are added in slot order, one tap at a time: thread r < cgb * 8 owns channel
    // (r / 8) * 8 + r % 8 of the workgroup's column
    const int rcg = t >> 3, ri = t & 7;
    const int rc = (blockIdx.y * p.cgb + rcg) * 8 + ri;
    float* dst = part + (size_t)blockIdx.x * p.C * 9 + (size_t)rc * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) sR[t * 8 + i] = acc[tap][i];
        __syncthreads();
        if (t < p.cgb * 8 && rc < p.C) {
            float a = 0.f;
            for (int sl = 0; sl < nslot; ++sl) a += sR[(sl * p.cgb + rcg) * 8 + ri];
            dst[tap] = a;
        }
    }
}

// pass 2: dw[e] = (accumulate ? dw[e] : 0) + sum_s part[s][e] for e < E
__global__ __launch_bounds__(256) void k_dw_wgrad_reduce(const float* __restrict__ part, int nsplit, long long E,
                                                         float* __restrict__ dw, int accumulate) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float a = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) a += part[(size_t)sp * E + e];
    dw[e] = accumulate ? dw[e] + a : a;
}

// ---------------------------------------------------------------------------------------------------------------------
// unit tail.  Logical channel c of the unit's output (c = 2 * j + g: g = 0 takes a[j], g = 1 takes b[j], j < bf) lives at
// physical channel (c / bf) * wp + c % bf of the 2 * wp wide row.  A thread writes 8 consecutive physical channels.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_tail_fwd(const T* __restrict__ a, long long lda, const T* __restrict__ b,
                                                  T* __restrict__ y, long long M, int bf, int wp) {
    const int G = 2 * wp / 8;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long m = idx / G;
    if (m >= M) return;
    const int p0 = (int)(idx - m * G) * 8;
    const int h = p0 / wp, i0 = p0 - h * wp;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = i0 + k;
        float f = 0.f;
        if (i < bf) {
            const int c = h * bf + i, j = c >> 1;
            f = (c & 1) ? load1<T>(b, (size_t)m * wp + j) : load1<T>(a, (size_t)m * lda + j);
        }
        v[k] = f;
    }
    store8<T>(y, (size_t)m * 2 * wp + p0, v);
}

// backward: da (M, aw) [channels >= bf zero] and db (M, wp) [channels >= bf zero] from dy (M, 2 * wp)
template <typename T>
__global__ __launch_bounds__(256) void k_tail_bwd(const T* __restrict__ dy, T* __restrict__ da, int aw, T* __restrict__ db,
                                                  long long M, int bf, int wp) {
    const int GA = aw / 8, G = GA + wp / 8;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long m = idx / G;
    if (m >= M) return;
    const int g = (int)(idx - m * G);
    const int which = g >= GA;
    const int j0 = (which ? g - GA : g) * 8;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int j = j0 + k;
        float f = 0.f;
        if (j < bf) {
            const int c = 2 * j + which;
            const int h = c >= bf;
            f = load1<T>(dy, (size_t)m * 2 * wp + h * wp + (c - h * bf));
        }
        v[k] = f;
    }
    if (which) store8<T>(db, (size_t)m * wp + j0, v);
    else store8<T>(da, (size_t)m * aw + j0, v);
}

// ---------------------------------------------------------------------------------------------------------------------
// pack / unpack.  Physical index i of a padded dimension maps to logical (i / wp) * wl + i % wp when i % wp < wl, and is a
// pad otherwise; along the columns the first col_skip halves are pads altogether.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_padded_pack(const cr_pdesc* __restrict__ descs, float* __restrict__ base,
                                                     float* __restrict__ baseT, int mode) {
    const cr_pdesc d = descs[blockIdx.y];
    float* __restrict__ lg = reinterpret_cast<float*>(d.logical);
    const long long total = (long long)d.rows_p * d.cols_p;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int pr = (int)(e / d.cols_p), pc = (int)(e - (long long)pr * d.cols_p);
        const int rh = pr / d.row_wp, ri = pr - rh * d.row_wp;
        const int ch = pc / d.col_wp - d.col_skip, ci = pc - (ch + d.col_skip) * d.col_wp;
        const bool valid = ri < d.row_wl && ci < d.col_wl && ch >= 0;
        const long long li = valid ? (long long)(rh * d.row_wl + ri) * d.cols_l + (ch * d.col_wl + ci) : 0;
        if (mode == 0) {
            const float v = valid ? lg[li] : 0.f;
            base[d.phys_off + e] = v;
            if (d.physT_off >= 0) baseT[d.physT_off + (long long)pc * d.rows_p + pr] = v;
        } else if (valid) {
            const float v = base[d.phys_off + e];
            lg[li] = mode == 2 ? lg[li] + v : v;
        }
    }
}

int check_dw(const char* who, int N, int H, int W, int C, int stride, int act_f32) {
    CR_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "%s: N, H, W must be >= 1 (got %d, %d, %d)", who, N, H, W);
    CR_CHECK_ARG(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (got %d)", who, stride);
    CR_CHECK_ARG(C >= 8 && C % 8 == 0, "%s: channels must be a positive multiple of 8 (got %d)", who, C);
    CR_CHECK_ARG(act_f32 >= 0 && act_f32 <= 2, "%s: act_f32 must be 0, 1 or 2 (got %d)", who, act_f32);
    return CR_OK;
}

DwP make_dw(int N, int H, int W, int C, int stride) {
    DwP p = {};
    p.N = N; p.H = H; p.W = W; p.C = C;
    p.Ho = (H - 1) / stride + 1;
    p.Wo = (W - 1) / stride + 1;
    int cgb = 1;
    while (cgb < 16 && cgb < C / 8) cgb *= 2;
    p.cgb = cgb;
    return p;
}

}  // namespace

extern "C" int cr_dwconv3x3_fwd(cr_ctx* ctx, const void* x, const float* w, void* y, int N, int H, int W, int C, int stride,
                                const float* bias, float* stats, int act_f32) {
    CR_CHECK_ARG(ctx && x && w && y, "cr_dwconv3x3_fwd: NULL pointer");
    if (int rc = check_dw("cr_dwconv3x3_fwd", N, H, W, C, stride, act_f32)) return rc;
    DwP p = make_dw(N, H, W, C, stride);
    p.x = x; p.w = w; p.y = y; p.bias = bias; p.stats = stats;
    p.M = (long long)N * p.Ho * p.Wo;
    const long long gx = cr_cdiv(cr_cdiv(p.M, 64), 16 / p.cgb);
    CR_CHECK_ARG(gx <= 0x7fffffffLL, "cr_dwconv3x3_fwd: too many output pixels (%lld)", p.M);
    const dim3 grid((unsigned)gx, (unsigned)cr_cdiv(C / 8, p.cgb));
    if (act_f32) {
        if (stride == 1) hipLaunchKernelGGL((k_dw_fwd<float, 1>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_dw_fwd<float, 2>), grid, dim3(256), 0, ctx->stream, p);
    } else {
        if (stride == 1) hipLaunchKernelGGL((k_dw_fwd<u16, 1>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_dw_fwd<u16, 2>), grid, dim3(256), 0, ctx->stream, p);
    }
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dwconv3x3_bwd_data(cr_ctx* ctx, const void* dy, const float* w, void* dx, int N, int H, int W, int C,
                                     int stride, int act_f32, const void* accumulate) {
    CR_CHECK_ARG(ctx && dy && w && dx, "cr_dwconv3x3_bwd_data: NULL pointer");
    if (int rc = check_dw("cr_dwconv3x3_bwd_data", N, H, W, C, stride, act_f32)) return rc;
    DwP p = make_dw(N, H, W, C, stride);
    p.x = dy; p.w = w; p.y = dx; p.acc = accumulate;
    p.M = (long long)N * H * W;
    const long long gx = cr_cdiv(cr_cdiv(p.M, 64), 16 / p.cgb);
    CR_CHECK_ARG(gx <= 0x7fffffffLL, "cr_dwconv3x3_bwd_data: too many input pixels (%lld)", p.M);
    const dim3 grid((unsigned)gx, (unsigned)cr_cdiv(C / 8, p.cgb));
    if (act_f32) {
        if (stride == 1) hipLaunchKernelGGL((k_dw_bwd_data<float, 1>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_dw_bwd_data<float, 2>), grid, dim3(256), 0, ctx->stream, p);
    } else {
        if (stride == 1) hipLaunchKernelGGL((k_dw_bwd_data<u16, 1>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_dw_bwd_data<u16, 2>), grid, dim3(256), 0, ctx->stream, p);
    }
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dwconv3x3_bwd_weight(cr_ctx* ctx, const void* dy, const void* x, float* dw, int N, int H, int W, int C,
                                       int stride, int accumulate, int act_f32, float* ws, int64_t ws_floats) {
    CR_CHECK_ARG(ctx && dy && x && dw && ws, "cr_dwconv3x3_bwd_weight: NULL pointer");
    if (int rc = check_dw("cr_dwconv3x3_bwd_weight", N, H, W, C, stride, act_f32)) return rc;
    DwP p = make_dw(N, H, W, C, stride);
    p.x = x; p.dy = dy;
    p.M = (long long)N * p.Ho * p.Wo;
    // pixel ranges of at least 64 output pixels, at most 128 of them: a function of the problem alone
    const long long range = cr_cdiv(p.M, 128) > 64 ? cr_cdiv(p.M, 128) : 64;
    const int nsplit = (int)cr_cdiv(p.M, range);
    const long long E = (long long)C * 9;
    CR_CHECK_ARG(ws_floats >= (int64_t)nsplit * E,
                 "cr_dwconv3x3_bwd_weight: workspace of %lld floats, %lld needed (splits * C * 9, splits = %d)",
                 (long long)ws_floats, (long long)nsplit * E, nsplit);
    const dim3 grid((unsigned)nsplit, (unsigned)cr_cdiv(C / 8, p.cgb));
    if (act_f32) {
        if (stride == 1) hipLaunchKernelGGL((k_dw_wgrad<float, 1>), grid, dim3(256), 0, ctx->stream, p, range, ws);
        else hipLaunchKernelGGL((k_dw_wgrad<float, 2>), grid, dim3(256), 0, ctx->stream, p, range, ws);
    } else {
        if (stride == 1) hipLaunchKernelGGL((k_dw_wgrad<u16, 1>), grid, dim3(256), 0, ctx->stream, p, range, ws);
        else hipLaunchKernelGGL((k_dw_wgrad<u16, 2>), grid, dim3(256), 0, ctx->stream, p, range, ws);
    }
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dw_wgrad_reduce, dim3((unsigned)cr_cdiv(E, 256)), dim3(256), 0, ctx->stream, ws, nsplit, E, dw,
                       accumulate);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_shuffle_tail_fwd(cr_ctx* ctx, const void* a, int64_t lda, const void* b, void* y, int64_t M, int bf, int wp,
                                   int act_f32) {
    CR_CHECK_ARG(ctx && a && b && y, "cr_shuffle_tail_fwd: NULL pointer");
    CR_CHECK_ARG(M >= 1 && bf >= 1 && wp >= bf && wp % 8 == 0 && lda >= bf,
                 "cr_shuffle_tail_fwd: need M >= 1, 1 <= bf <= wp, wp %% 8 == 0, lda >= bf (got M %lld, bf %d, wp %d, lda %lld)",
                 (long long)M, bf, wp, (long long)lda);
    const long long blocks = cr_cdiv((long long)M * (2 * wp / 8), 256);
    CR_CHECK_ARG(blocks <= 0x7fffffffLL, "cr_shuffle_tail_fwd: too many pixels (%lld)", (long long)M);
    if (act_f32) hipLaunchKernelGGL(k_tail_fwd<float>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const float*)a,
                                    (long long)lda, (const float*)b, (float*)y, (long long)M, bf, wp);
    else hipLaunchKernelGGL(k_tail_fwd<u16>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const u16*)a, (long long)lda,
                            (const u16*)b, (u16*)y, (long long)M, bf, wp);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_shuffle_tail_bwd(cr_ctx* ctx, const void* dy, void* da, int aw, void* db, int64_t M, int bf, int wp,
                                   int act_f32) {
    CR_CHECK_ARG(ctx && dy && da && db, "cr_shuffle_tail_bwd: NULL pointer");
    CR_CHECK_ARG(M >= 1 && bf >= 1 && wp >= bf && wp % 8 == 0 && aw >= bf && aw % 8 == 0,
                 "cr_shuffle_tail_bwd: need M >= 1, 1 <= bf <= wp, wp %% 8 == 0, aw >= bf, aw %% 8 == 0 (got M %lld, bf %d, wp %d, "
                 "aw %d)", (long long)M, bf, wp, aw);
    const long long blocks = cr_cdiv((long long)M * ((aw + wp) / 8), 256);
    CR_CHECK_ARG(blocks <= 0x7fffffffLL, "cr_shuffle_tail_bwd: too many pixels (%lld)", (long long)M);
    if (act_f32) hipLaunchKernelGGL(k_tail_bwd<float>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const float*)dy,
                                    (float*)da, aw, (float*)db, (long long)M, bf, wp);
    else hipLaunchKernelGGL(k_tail_bwd<u16>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const u16*)dy, (u16*)da, aw,
                            (u16*)db, (long long)M, bf, wp);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_padded_pack(cr_ctx* ctx, const void* descs_dev, int ndesc, float* base, float* baseT, int mode) {
    CR_CHECK_ARG(ctx && descs_dev && base, "cr_padded_pack: NULL pointer");
    CR_CHECK_ARG(ndesc >= 1 && ndesc <= 65535, "cr_padded_pack: 1 <= ndesc <= 65535 (got %d)", ndesc);
    CR_CHECK_ARG(mode >= 0 && mode <= 2, "cr_padded_pack: mode must be 0, 1 or 2 (got %d)", mode);
    hipLaunchKernelGGL(k_padded_pack, dim3(16, (unsigned)ndesc), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const cr_pdesc*>(descs_dev), base, baseT, mode);
    CR_LAUNCH_CHECK();
    return CR_OK;
}
