// MNASNet trunk kernels (cubercnn/modeling/backbone/mnasnet.py of the reference takes torchvision's mnasnet1_0): memory-bound
// vector-ALU work in plain C++, no atomics, 64-bit element offsets, predicated halos, grids that follow from the problem size.
//
//   * depthwise k x k convolution, k in {3, 5}, pad k / 2, stride 1 or 2: cr_dwconv_fwd / _bwd_data / _bwd_weight.  With 8
//     channels per thread (the 3x3 plan of csrc/shufflenet.hip: 72 tap weights in registers) the 25 taps of a 5x5 would need
//     200 weight registers (200 accumulators in the weight gradient), so a 5x5 thread owns FOUR consecutive channels -- 100
//     weight registers / accumulators, one 16-byte load per tap in f32 and one 8-byte load in bf16 -- and 4 consecutive
//     pixels.  Everything else is the 3x3 plan: consecutive lanes are consecutive channel groups, the forward can emit
//     BatchNorm statistics rows in cr_bn_fwd's layout (one row per 64 output pixels, summed in a fixed order), the weight
//     gradient is two passes through the caller's workspace.  The forward is one template over k (it adds a ReLU epilogue
//     that cr_dwconv3x3_fwd does not have); backward-data and the weight gradient of k = 3 ARE cr_dwconv3x3_bwd_*.
//   * BatchNorm backward for any C % 8 == 0 (cr_bn_bwd_anyc): cr_bn_bwd / cr_bn_bwd_mask need 256 % (C / 8) == 0.  Here a
//     workgroup owns a slice of 32 channels (4 threads x 8 channels per pixel, 64 pixels per pass) and a pixel chunk; channel
//     groups beyond C are predicated off, so nothing depends on how C / 8 relates to the workgroup size.  Per-channel sums
//     add a thread's pixels in float32 and everything across threads in double; cr_colsum_wide is the same plan for a plain
//     column sum (the bias gradient of the frozen backward).
#include "cr_common.h"
#include "cr_elem.h"
#include "cr3dod.h"

namespace {

template <typename T> __device__ __forceinline__ float as_stored(float v) {
    if constexpr (sizeof(T) == 4) return v; else return bf2f(f2bf(v));
}

constexpr int V5 = 4;        // channels per thread of the 5x5 kernels
constexpr int T5 = 25;       // taps

struct Dw5P {
    const void* x;       // forward: input; backward-data: dy; weight gradient: x
    const void* dy;      // weight gradient only
    const float* w;      // (C, k, k)
    void* y;             // forward: output; backward-data: dx
    const float* bias;
    const void* acc;     // backward-data: accumulate
    float* stats;
    int N, H, W, Ho, Wo, C;
    int cgb;             // channel groups (of V channels) per workgroup: a power of two <= 16
    long long M;         // pixels the grid runs over
};

// the K * K taps of V consecutive channels: w[(c0 + i) * K * K + tap] -> wv[tap][i]  (V * K * K consecutive floats, 16-byte
// aligned: 72 for K = 3 / V = 8, 100 for K = 5 / V = 4)
template <int K, int V> __device__ __forceinline__ void load_taps(const float* __restrict__ w, int c0, float (*wv)[V]) {
    constexpr int KK = K * K;
    float wl[V * KK];
    const float4* src = reinterpret_cast<const float4*>(w + (size_t)c0 * KK);
#pragma unroll
    for (int i = 0; i < V * KK / 4; ++i) {
        const float4 v = src[i];
        wl[4 * i] = v.x; wl[4 * i + 1] = v.y; wl[4 * i + 2] = v.z; wl[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int tap = 0; tap < KK; ++tap)
#pragma unroll
        for (int i = 0; i < V; ++i) wv[tap][i] = wl[i * KK + tap];
}

// forward, K = 3 (V = 8 channels per thread, the plan of cr_dwconv3x3_fwd) or K = 5 (V = 4), with an optional ReLU in the
// epilogue (the folded BatchNorm + ReLU of frozen / eval mode).  Thread t of a 256-thread workgroup: channel group t % cgb,
// pixel quad (t / cgb) % 16, row t / (16 * cgb) of the 16 / cgb rows of 64 pixels the workgroup covers
template <typename T, int K, int STRIDE>
__global__ __launch_bounds__(256) void k_dwk_fwd(const Dw5P p, int relu) {
    constexpr int V = K == 3 ? 8 : 4, KK = K * K;
    __shared__ float sS[512 * V];                            // [row][quad][2][cgb * V]
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    T* __restrict__ y = reinterpret_cast<T*>(p.y);
    const int t = threadIdx.x;
    const int cgi = t % p.cgb, quad = (t / p.cgb) & 15, row = t / (p.cgb * 16);
    const int rb = 16 / p.cgb;
    const int c0 = (blockIdx.y * p.cgb + cgi) * V;
    const bool cok = c0 < p.C;
    const long long rowi = (long long)blockIdx.x * rb + row;
    const long long q0 = rowi * 64 + quad * 4;
    float ssum[V], ssq[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { ssum[i] = 0.f; ssq[i] = 0.f; }
    if (cok && q0 < p.M) {
        float wv[KK][V], bias[V];
        load_taps<K, V>(p.w, c0, wv);
#pragma unroll
        for (int i = 0; i < V; ++i) bias[i] = p.bias ? p.bias[c0 + i] : 0.f;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const long long q = q0 + j;
            if (q >= p.M) break;
            const int wo = (int)(q % p.Wo);
            const long long tq = q / p.Wo;
            const int ho = (int)(tq % p.Ho), n = (int)(tq / p.Ho);
            float acc[V];
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] = bias[i];
#pragma unroll
            for (int tap = 0; tap < KK; ++tap) {
                const int r = tap / K, s = tap - r * K;
                const int hi = ho * STRIDE + r - K / 2, wi = wo * STRIDE + s - K / 2;
                if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
                    float xv[V];
                    loadv<T, V>(x, (((size_t)n * p.H + hi) * p.W + wi) * p.C + c0, xv);
#pragma unroll
                    for (int i = 0; i < V; ++i) acc[i] = fmaf(xv[i], wv[tap][i], acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (relu) acc[i] = fmaxf(acc[i], 0.f);
                const float vs = as_stored<T>(acc[i]);       // statistics are those of the values BatchNorm will read
                ssum[i] += vs;
                ssq[i] = fmaf(vs, vs, ssq[i]);
            }
            storev<T, V>(y, (size_t)q * p.C + c0, acc);
        }
    }
    if (p.stats == nullptr) return;                          // block-uniform
    const int cw = p.cgb * V;
    {
        float* d0 = sS + ((size_t)((row * 16 + quad) * 2 + 0) * p.cgb + cgi) * V;
        float* d1 = d0 + cw;
#pragma unroll
        for (int i = 0; i < V; ++i) { d0[i] = ssum[i]; d1[i] = ssq[i]; }
    }
    __syncthreads();
    if (quad < 2 && cok && rowi * 64 < p.M) {                // quad = which (0: sum, 1: sum of squares)
        float a[V];
#pragma unroll
        for (int i = 0; i < V; ++i) a[i] = 0.f;
        for (int qd = 0; qd < 16; ++qd) {                    // fixed order
            const float* s = sS + ((size_t)((row * 16 + qd) * 2 + quad) * p.cgb + cgi) * V;
#pragma unroll
            for (int i = 0; i < V; ++i) a[i] += s[i];
        }
        storev<float, V>(p.stats, ((size_t)rowi * 2 + quad) * p.C + c0, a);
    }
}

// backward-data: dx[n,h,w,c] = sum over taps (r,s) with ho * stride + r - 2 == h (same for w) of dy[n,ho,wo,c] * w[c][r][s]
// (+ accumulate); the grid runs over input pixels
template <typename T, int STRIDE>
__global__ __launch_bounds__(256) void k_dw5_bwd_data(const Dw5P p) {
    const T* __restrict__ dy = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ acc_in = reinterpret_cast<const T*>(p.acc);
    T* __restrict__ dx = reinterpret_cast<T*>(p.y);
    const int t = threadIdx.x;
    const int cgi = t % p.cgb, quad = (t / p.cgb) & 15, row = t / (p.cgb * 16);
    const int rb = 16 / p.cgb;
    const int c0 = (blockIdx.y * p.cgb + cgi) * V5;
    const long long q0 = ((long long)blockIdx.x * rb + row) * 64 + quad * 4;
    if (c0 >= p.C || q0 >= p.M) return;
    float wv[T5][V5];
    load_taps<5, V5>(p.w, c0, wv);
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const long long q = q0 + j;
        if (q >= p.M) break;
        const int wq = (int)(q % p.W);
        const long long tq = q / p.W;
        const int h = (int)(tq % p.H), n = (int)(tq / p.H);
        float acc[V5];
#pragma unroll
        for (int i = 0; i < V5; ++i) acc[i] = 0.f;
        if (acc_in) load4<T>(acc_in, (size_t)q * p.C + c0, acc);
#pragma unroll
        for (int tap = 0; tap < T5; ++tap) {
            const int r = tap / 5, s = tap - r * 5;
            const int th = h + 2 - r, tw = wq + 2 - s;
            bool in = th >= 0 && tw >= 0;
            int ho = th, wo = tw;
            if (STRIDE == 2) {
                in = in && ((th & 1) == 0) && ((tw & 1) == 0);
                ho = th >> 1;
                wo = tw >> 1;
            }
            if (in && ho < p.Ho && wo < p.Wo) {
                float gv[V5];
                load4<T>(dy, (((size_t)n * p.Ho + ho) * p.Wo + wo) * p.C + c0, gv);
#pragma unroll
                for (int i = 0; i < V5; ++i) acc[i] = fmaf(gv[i], wv[tap][i], acc[i]);
            }
        }
        store4<T>(dx, (size_t)q * p.C + c0, acc);
    }
}

// weight gradient, pass 1: workgroup blockIdx.x owns the output pixels [split * range, (split + 1) * range); thread t =
// channel group t % cgb, slot t / cgb takes every (256 / cgb)-th pixel of the range; the slots are added in slot order
// through LDS, one tap at a time, and the workgroup writes the partial dw of its range into part[split][C * 25].  Pass 2 adds
// the ranges in index order.
template <typename T, int STRIDE>
__global__ __launch_bounds__(256) void k_dw5_wgrad(const Dw5P p, long long range, float* __restrict__ part) {
    __shared__ float sR[256 * V5];
    const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
    const T* __restrict__ dy = reinterpret_cast<const T*>(p.dy);
    const int t = threadIdx.x;
    const int cgi = t % p.cgb, slot = t / p.cgb, nslot = 256 / p.cgb;
    const int c0 = (blockIdx.y * p.cgb + cgi) * V5;
    const bool cok = c0 < p.C;
    const long long q0 = (long long)blockIdx.x * range;
    const long long q1 = (q0 + range < p.M) ? q0 + range : p.M;
    float acc[T5][V5];
#pragma unroll
    for (int tap = 0; tap < T5; ++tap)
#pragma unroll
        for (int i = 0; i < V5; ++i) acc[tap][i] = 0.f;
    if (cok) {
        for (long long q = q0 + slot; q < q1; q += nslot) {
            const int wo = (int)(q % p.Wo);
            const long long tq = q / p.Wo;
            const int ho = (int)(tq % p.Ho), n = (int)(tq / p.Ho);
            float g[V5];
            load4<T>(dy, (size_t)q * p.C + c0, g);
#pragma unroll
            for (int tap = 0; tap < T5; ++tap) {
                const int r = tap / 5, s = tap - r * 5;
                const int hi = ho * STRIDE + r - 2, wi = wo * STRIDE + s - 2;
                if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W) {
                    float xv[V5];
                    load4<T>(x, (((size_t)n * p.H + hi) * p.W + wi) * p.C + c0, xv);
#pragma unroll
                    for (int i = 0; i < V5; ++i) acc[tap][i] = fmaf(g[i], xv[i], acc[tap][i]);
                }
            }
        }
    }
    // thread r < cgb * 4 owns channel (r / 4) * 4 + r % 4 of the workgroup's column
    const int rcg = t / V5, ri = t % V5;
    const int rc = (blockIdx.y * p.cgb + rcg) * V5 + ri;
    float* dst = part + (size_t)blockIdx.x * p.C * T5 + (size_t)rc * T5;
#pragma unroll
    for (int tap = 0; tap < T5; ++tap) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < V5; ++i) sR[t * V5 + i] = acc[tap][i];
        __syncthreads();
        if (t < p.cgb * V5 && rc < p.C) {
            float a = 0.f;
            for (int sl = 0; sl < nslot; ++sl) a += sR[(sl * p.cgb + rcg) * V5 + ri];
            dst[tap] = a;
        }
    }
}

// pass 2: dw[e] = (accumulate ? dw[e] : 0) + sum_s part[s][e] for e < E
__global__ __launch_bounds__(256) void k_dw5_wgrad_reduce(const float* __restrict__ part, int nsplit, long long E,
                                                          float* __restrict__ dw, int accumulate) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float a = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) a += part[(size_t)sp * E + e];
    dw[e] = accumulate ? dw[e] + a : a;
}

int check_dw(const char* who, int N, int H, int W, int C, int k, int stride, int act_f32) {
    CR_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "%s: N, H, W must be >= 1 (got %d, %d, %d)", who, N, H, W);
    CR_CHECK_ARG(k == 3 || k == 5, "%s: k must be 3 or 5 (got %d)", who, k);
    CR_CHECK_ARG(stride == 1 || stride == 2, "%s: stride must be 1 or 2 (got %d)", who, stride);
    CR_CHECK_ARG(C >= 8 && C % 8 == 0, "%s: channels must be a positive multiple of 8 (got %d)", who, C);
    CR_CHECK_ARG(act_f32 >= 0 && act_f32 <= 2, "%s: act_f32 must be 0, 1 or 2 (got %d)", who, act_f32);
    return CR_OK;
}

Dw5P make_dw(int N, int H, int W, int C, int stride, int V) {
    Dw5P p = {};
    p.N = N; p.H = H; p.W = W; p.C = C;
    p.Ho = (H - 1) / stride + 1;
    p.Wo = (W - 1) / stride + 1;
    int cgb = 1;
    while (cgb < 16 && cgb < C / V) cgb *= 2;
    p.cgb = cgb;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm backward, any C % 8 == 0.  g = dy * mask, xh = (x - mean) * invstd:
//   dbeta += sum g, dgamma += sum g * xh, dx = gamma * invstd * (g - sum g / M - xh * sum g xh / M)
// ---------------------------------------------------------------------------------------------------------------------
// The forward's value before the ReLU in the form cr_bn_fwd computes it (csrc/conv.hip, bn_affine): subtract, multiply, then
// ONE fused multiply-add -- the mask taken from x must have the bits of the value the forward stored.
__device__ __forceinline__ float bna_affine(float x, float mean, float invstd, float gamma, float beta) {
#pragma clang fp contract(off)
    const float xh = (x - mean) * invstd;
    return __builtin_fmaf(xh, gamma, beta);
}
template <typename T> __device__ __forceinline__ bool bna_relu_on(float v) { return as_stored<T>(fmaxf(v, 0.f)) > 0.f; }

// pass 1: workgroup (pixel chunk bx, channel slice by of 32): thread t = channel group t & 3 of the slice, pixel lane t >> 2;
// the 64 pixel lanes are added in lane order through LDS (in double) -> partial[bx][2][C] (sum g, sum g * xh)
template <typename T, bool MASKX>
__global__ __launch_bounds__(256) void k_bna_reduce(const T* __restrict__ dy, const T* __restrict__ out,
                                                    const T* __restrict__ x, const float* __restrict__ mean_invstd,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float* __restrict__ partial, long long M, int C, int relu, int ppb) {
    __shared__ float s_acc[64 * 2 * 32];
    const int t = threadIdx.x, cgl = t & 3, lane = t >> 2;
    const int cbase = blockIdx.y * 32, c0 = cbase + cgl * 8;
    float a[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = 0.f; b[e] = 0.f; }
    if (c0 < C) {
        float mu[8], is[8], ga[8], be[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mu[e] = mean_invstd[c0 + e]; is[e] = mean_invstd[C + c0 + e];
            ga[e] = MASKX ? gamma[c0 + e] : 0.f; be[e] = MASKX ? beta[c0 + e] : 0.f;
        }
        const long long m0 = (long long)blockIdx.x * ppb, m1 = m0 + ppb < M ? m0 + ppb : M;
        for (long long m = m0 + lane; m < m1; m += 64) {
            const size_t i8 = (size_t)m * C + c0;
            float dv[8], xv[8], ov[8];
            load8<T>(dy, i8, dv);
            load8<T>(x, i8, xv);
            if (relu && !MASKX) load8<T>(out, i8, ov);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool on = MASKX ? bna_relu_on<T>(bna_affine(xv[e], mu[e], is[e], ga[e], be[e])) : (!relu || ov[e] > 0.f);
                const float gq = on ? dv[e] : 0.f;
                const float xh = (xv[e] - mu[e]) * is[e];
                a[e] += gq;
                b[e] += gq * xh;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s_acc[(lane * 2 + 0) * 32 + cgl * 8 + e] = a[e];
        s_acc[(lane * 2 + 1) * 32 + cgl * 8 + e] = b[e];
    }
    __syncthreads();
    if (t < 64) {
        const int which = t >> 5, ch = t & 31;
        if (cbase + ch < C) {
            double s = 0.0;                              // the lanes' sums cancel: add them in double, round once
            for (int r = 0; r < 64; ++r) s += (double)s_acc[(r * 2 + which) * 32 + ch];      // fixed order
            partial[((size_t)blockIdx.x * 2 + which) * C + cbase + ch] = (float)s;
        }
    }
}

// pass 2: every workgroup of a slice first adds the nparts partial rows of ITS 32 channels (8 row lanes per channel, double,
// fixed order: the same bits in every workgroup of the slice), then writes dx for its pixel chunk; the workgroups of chunk 0
// accumulate dgamma / dbeta
template <typename T, bool MASKX>
__global__ __launch_bounds__(256) void k_bna_apply(const T* __restrict__ dy, const T* __restrict__ out, const T* __restrict__ x,
                                                   const float* __restrict__ mean_invstd, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ partial,
                                                   int nparts, T* __restrict__ dx, float* __restrict__ dgamma,
                                                   float* __restrict__ dbeta, long long M, int C, int relu, int ppb) {
    __shared__ double sd[2][8][32];
    __shared__ float sc[4][32];                          // mean, invstd, sum_g / M, sum_gx / M
    const int t = threadIdx.x, ch = t & 31, rl = t >> 5;
    const int cbase = blockIdx.y * 32, c = cbase + ch;
    {
        double s = 0.0, q = 0.0;
        if (c < C) {
            for (int r = rl; r < nparts; r += 8) {
                s += (double)partial[(size_t)r * 2 * C + c];
                q += (double)partial[(size_t)r * 2 * C + C + c];
            }
        }
        sd[0][rl][ch] = s; sd[1][rl][ch] = q;
    }
    __syncthreads();
    if (t < 32) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r) { s += sd[0][r][t]; q += sd[1][r][t]; }
        const float sg = (float)s, sgx = (float)q, invM = 1.f / (float)M;
        const bool ok = cbase + t < C;
        sc[0][t] = ok ? mean_invstd[cbase + t] : 0.f;
        sc[1][t] = ok ? mean_invstd[C + cbase + t] : 0.f;
        sc[2][t] = sg * invM;
        sc[3][t] = sgx * invM;
        if (ok && blockIdx.x == 0) { dbeta[cbase + t] += sg; dgamma[cbase + t] += sgx; }
    }
    __syncthreads();
    const int cgl = t & 3, c0 = cbase + cgl * 8;
    if (c0 >= C) return;
    float mu[8], is8[8], ga[8], be[8], k1[8], k2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int cc = cgl * 8 + e;
        mu[e] = sc[0][cc]; is8[e] = sc[1][cc]; ga[e] = gamma[c0 + e]; k1[e] = sc[2][cc]; k2[e] = sc[3][cc];
        be[e] = MASKX ? beta[c0 + e] : 0.f;
    }
    const long long m0 = (long long)blockIdx.x * ppb, m1 = m0 + ppb < M ? m0 + ppb : M;
    for (long long m = m0 + (t >> 2); m < m1; m += 64) {
        const size_t i8 = (size_t)m * C + c0;
        float dv[8], xv[8], ov[8], vd[8];
        load8<T>(dy, i8, dv);
        load8<T>(x, i8, xv);
        if (relu && !MASKX) load8<T>(out, i8, ov);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool on = MASKX ? bna_relu_on<T>(bna_affine(xv[e], mu[e], is8[e], ga[e], be[e])) : (!relu || ov[e] > 0.f);
            const float gq = on ? dv[e] : 0.f;
            const float xh = (xv[e] - mu[e]) * is8[e];
            vd[e] = ga[e] * is8[e] * (gq - k1[e] - xh * k2[e]);
        }
        store8<T>(dx, i8, vd);
    }
}

// per-channel sums out[c] += sum_m x[m][c] with the plan of k_bna_reduce: a thread adds its pixels in float32, the 64 lanes are
// added in lane order in double -> partial[bx][C]; k_cs_final adds the chunks in index order in double.
template <typename T>
__global__ __launch_bounds__(256) void k_cs_reduce(const T* __restrict__ x, float* __restrict__ partial, long long M, int C,
                                                   int ppb) {
    __shared__ float s_acc[64 * 32];
    const int t = threadIdx.x, cgl = t & 3, lane = t >> 2;
    const int cbase = blockIdx.y * 32, c0 = cbase + cgl * 8;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    if (c0 < C) {
        const long long m0 = (long long)blockIdx.x * ppb, m1 = m0 + ppb < M ? m0 + ppb : M;
        for (long long m = m0 + lane; m < m1; m += 64) {
            float xv[8];
            load8<T>(x, (size_t)m * C + c0, xv);
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += xv[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_acc[lane * 32 + cgl * 8 + e] = a[e];
    __syncthreads();
    if (t < 32 && cbase + t < C) {
        double s = 0.0;
        for (int r = 0; r < 64; ++r) s += (double)s_acc[r * 32 + t];                 // fixed order
        partial[(size_t)blockIdx.x * C + cbase + t] = (float)s;
    }
}

__global__ __launch_bounds__(256) void k_cs_final(const float* __restrict__ partial, int nparts, int C, float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int r = 0; r < nparts; ++r) s += (double)partial[(size_t)r * C + c];        // fixed order
    out[c] += (float)s;
}

template <typename T, bool MASKX>
int bna_launch(cr_ctx* ctx, const T* dy, const T* out, const T* x, const float* mean_invstd, const float* gamma,
               const float* beta, float* ws, T* dx, float* dgamma, float* dbeta, long long M, int C, int relu) {
    // pixel chunks of at least 256 pixels (a multiple of 64), at most 256 of them: a function of M alone
    long long nb = cr_cdiv(M, 256);
    if (nb > 256) nb = 256;
    long long ppb = cr_cdiv(cr_cdiv(M, nb), 64) * 64;
    nb = cr_cdiv(M, ppb);
    CR_CHECK_ARG(ppb <= 0x7fffffffLL, "cr_bn_bwd_anyc: too many pixels (%lld)", M);
    const dim3 grid((unsigned)nb, (unsigned)cr_cdiv(C, 32));
    hipLaunchKernelGGL((k_bna_reduce<T, MASKX>), grid, dim3(256), 0, ctx->stream, dy, out, x, mean_invstd, gamma, beta, ws, M, C,
                       relu, (int)ppb);
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_bna_apply<T, MASKX>), grid, dim3(256), 0, ctx->stream, dy, out, x, mean_invstd, gamma, beta, ws,
                       (int)nb, dx, dgamma, dbeta, M, C, relu, (int)ppb);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

}  // namespace

extern "C" int cr_dwconv_fwd(cr_ctx* ctx, const void* x, const float* w, void* y, int N, int H, int W, int C, int k, int stride,
                             const float* bias, float* stats, int relu, int act_f32) {
    CR_CHECK_ARG(ctx && x && w && y, "cr_dwconv_fwd: NULL pointer");
    if (int rc = check_dw("cr_dwconv_fwd", N, H, W, C, k, stride, act_f32)) return rc;
    CR_CHECK_ARG(relu == 0 || relu == 1, "cr_dwconv_fwd: relu must be 0 or 1 (got %d)", relu);
    const int V = k == 3 ? 8 : V5;
    Dw5P p = make_dw(N, H, W, C, stride, V);
    p.x = x; p.w = w; p.y = y; p.bias = bias; p.stats = stats;
    p.M = (long long)N * p.Ho * p.Wo;
    const long long gx = cr_cdiv(cr_cdiv(p.M, 64), 16 / p.cgb);
    CR_CHECK_ARG(gx <= 0x7fffffffLL, "cr_dwconv_fwd: too many output pixels (%lld)", p.M);
    const dim3 grid((unsigned)gx, (unsigned)cr_cdiv(C / V, p.cgb));
#define CR_DWK_FWD(T, K, S) hipLaunchKernelGGL((k_dwk_fwd<T, K, S>), grid, dim3(256), 0, ctx->stream, p, relu)
    if (act_f32) {
        if (k == 3) { if (stride == 1) CR_DWK_FWD(float, 3, 1); else CR_DWK_FWD(float, 3, 2); }
        else { if (stride == 1) CR_DWK_FWD(float, 5, 1); else CR_DWK_FWD(float, 5, 2); }
    } else {
        if (k == 3) { if (stride == 1) CR_DWK_FWD(u16, 3, 1); else CR_DWK_FWD(u16, 3, 2); }
        else { if (stride == 1) CR_DWK_FWD(u16, 5, 1); else CR_DWK_FWD(u16, 5, 2); }
    }
#undef CR_DWK_FWD
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dwconv_bwd_data(cr_ctx* ctx, const void* dy, const float* w, void* dx, int N, int H, int W, int C, int k,
                                  int stride, int act_f32, const void* accumulate) {
    CR_CHECK_ARG(ctx && dy && w && dx, "cr_dwconv_bwd_data: NULL pointer");
    if (int rc = check_dw("cr_dwconv_bwd_data", N, H, W, C, k, stride, act_f32)) return rc;
    if (k == 3) return cr_dwconv3x3_bwd_data(ctx, dy, w, dx, N, H, W, C, stride, act_f32, accumulate);
    Dw5P p = make_dw(N, H, W, C, stride, V5);
    p.x = dy; p.w = w; p.y = dx; p.acc = accumulate;
    p.M = (long long)N * H * W;
    const long long gx = cr_cdiv(cr_cdiv(p.M, 64), 16 / p.cgb);
    CR_CHECK_ARG(gx <= 0x7fffffffLL, "cr_dwconv_bwd_data: too many input pixels (%lld)", p.M);
    const dim3 grid((unsigned)gx, (unsigned)cr_cdiv(C / V5, p.cgb));
    if (act_f32) {
        if (stride == 1) hipLaunchKernelGGL((k_dw5_bwd_data<float, 1>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_dw5_bwd_data<float, 2>), grid, dim3(256), 0, ctx->stream, p);
    } else {
        if (stride == 1) hipLaunchKernelGGL((k_dw5_bwd_data<u16, 1>), grid, dim3(256), 0, ctx->stream, p);
        else hipLaunchKernelGGL((k_dw5_bwd_data<u16, 2>), grid, dim3(256), 0, ctx->stream, p);
    }
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_dwconv_bwd_weight(cr_ctx* ctx, const void* dy, const void* x, float* dw, int N, int H, int W, int C, int k,
                                    int stride, int accumulate, int act_f32, float* ws, int64_t ws_floats) {
    CR_CHECK_ARG(ctx && dy && x && dw && ws, "cr_dwconv_bwd_weight: NULL pointer");
    if (int rc = check_dw("cr_dwconv_bwd_weight", N, H, W, C, k, stride, act_f32)) return rc;
    if (k == 3) return cr_dwconv3x3_bwd_weight(ctx, dy, x, dw, N, H, W, C, stride, accumulate, act_f32, ws, ws_floats);
    Dw5P p = make_dw(N, H, W, C, stride, V5);
    p.x = x; p.dy = dy;
    p.M = (long long)N * p.Ho * p.Wo;
    // pixel ranges of at least 64 output pixels, at most 128 of them: a function of the problem alone
    const long long range = cr_cdiv(p.M, 128) > 64 ? cr_cdiv(p.M, 128) : 64;
    const int nsplit = (int)cr_cdiv(p.M, range);
    const long long E = (long long)C * T5;
    CR_CHECK_ARG(ws_floats >= (int64_t)nsplit * E,
                 "cr_dwconv_bwd_weight: workspace of %lld floats, %lld needed (splits * C * k * k, splits = %d)",
                 (long long)ws_floats, (long long)nsplit * E, nsplit);
    const dim3 grid((unsigned)nsplit, (unsigned)cr_cdiv(C / V5, p.cgb));
    if (act_f32) {
        if (stride == 1) hipLaunchKernelGGL((k_dw5_wgrad<float, 1>), grid, dim3(256), 0, ctx->stream, p, range, ws);
        else hipLaunchKernelGGL((k_dw5_wgrad<float, 2>), grid, dim3(256), 0, ctx->stream, p, range, ws);
    } else {
        if (stride == 1) hipLaunchKernelGGL((k_dw5_wgrad<u16, 1>), grid, dim3(256), 0, ctx->stream, p, range, ws);
        else hipLaunchKernelGGL((k_dw5_wgrad<u16, 2>), grid, dim3(256), 0, ctx->stream, p, range, ws);
    }
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dw5_wgrad_reduce, dim3((unsigned)cr_cdiv(E, 256)), dim3(256), 0, ctx->stream, ws, nsplit, E, dw,
                       accumulate);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_bn_bwd_anyc(cr_ctx* ctx, const void* dy, const void* out, const void* x, const float* mean_invstd,
                              const float* gamma, const float* beta, float* ws, void* dx, float* dgamma, float* dbeta,
                              int64_t M, int C, int relu, int act_f32) {
    CR_CHECK_ARG(ctx && dy && x && mean_invstd && gamma && beta && ws && dx && dgamma && dbeta, "cr_bn_bwd_anyc: NULL pointer");
    CR_CHECK_ARG(relu == 0 || relu == 1, "cr_bn_bwd_anyc: relu must be 0 or 1 (got %d)", relu);
    CR_CHECK_ARG(M > 0 && C >= 8 && C % 8 == 0 && C <= 2048, "cr_bn_bwd_anyc: unsupported M=%lld C=%d (C %% 8 == 0, C <= 2048)",
                 (long long)M, C);
    const bool maskx = relu && !out;
    if (act_f32) {
        if (maskx) return bna_launch<float, true>(ctx, (const float*)dy, nullptr, (const float*)x, mean_invstd, gamma, beta, ws,
                                                  (float*)dx, dgamma, dbeta, M, C, relu);
        return bna_launch<float, false>(ctx, (const float*)dy, (const float*)out, (const float*)x, mean_invstd, gamma, beta, ws,
                                        (float*)dx, dgamma, dbeta, M, C, relu);
    }
    if (maskx) return bna_launch<u16, true>(ctx, (const u16*)dy, nullptr, (const u16*)x, mean_invstd, gamma, beta, ws, (u16*)dx,
                                            dgamma, dbeta, M, C, relu);
    return bna_launch<u16, false>(ctx, (const u16*)dy, (const u16*)out, (const u16*)x, mean_invstd, gamma, beta, ws, (u16*)dx,
                                  dgamma, dbeta, M, C, relu);
}

extern "C" int cr_colsum_wide(cr_ctx* ctx, const void* x, int64_t M, int C, float* ws, float* out, int act_f32) {
    CR_CHECK_ARG(ctx && x && ws && out, "cr_colsum_wide: NULL pointer");
    CR_CHECK_ARG(M > 0 && C >= 8 && C % 8 == 0, "cr_colsum_wide: unsupported M=%lld C=%d (C %% 8 == 0)", (long long)M, C);
    long long nb = cr_cdiv(M, 256);                      // the chunks of cr_bn_bwd_anyc
    if (nb > 256) nb = 256;
    const long long ppb = cr_cdiv(cr_cdiv(M, nb), 64) * 64;
    nb = cr_cdiv(M, ppb);
    CR_CHECK_ARG(ppb <= 0x7fffffffLL, "cr_colsum_wide: too many rows (%lld)", (long long)M);
    const dim3 grid((unsigned)nb, (unsigned)cr_cdiv(C, 32));
    if (act_f32) hipLaunchKernelGGL(k_cs_reduce<float>, grid, dim3(256), 0, ctx->stream, (const float*)x, ws, (long long)M, C, (int)ppb);
    else hipLaunchKernelGGL(k_cs_reduce<u16>, grid, dim3(256), 0, ctx->stream, (const u16*)x, ws, (long long)M, C, (int)ppb);
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cs_final, dim3((unsigned)cr_cdiv(C, 256)), dim3(256), 0, ctx->stream, ws, (int)nb, C, out);
    CR_LAUNCH_CHECK();
    return CR_OK;
}
