// GroupNorm over NHWC maps, forward and backward, f32 and bf16 (torch.nn.GroupNorm(G, C) of detectron2's FPN norm "GN" and of
// its conv box head; optional ReLU after it).  Memory-bound vector-ALU work in plain C++.
//
// Nothing gathers a group.  Everything GroupNorm needs follows from per-(sample, channel) sums over pixels:
//   forward   S_x = sum x, S_xx = sum x^2                      -> mu, r = 1 / sqrt(var + eps) per (sample, group)
//   backward  S_g = sum g, S_gx = sum g * (x - mu)             (g = dy, masked by the stored output y > 0 with ReLU)
//             m1 = mean_group(gamma * g) = sum_c gamma_c S_g / count,   m2 = mean_group(gamma * g * xhat) = r sum_c gamma_c S_gx / count
//   y  = (x - mu) * (gamma r) + beta                            (x - mu first: a constant group gives exactly beta)
//   dx = (gamma r) g + B (x - mu) + D,   B = -r^2 m2,   D = -r m1
//   dgamma_c = sum_n r_n S_gx[n, c],   dbeta_c = sum_n S_g[n, c]
// A thread owns V = 4 (f32) or 8 (bf16) consecutive channels -- one 16-byte access -- and walks pixels.  Sums over pixels
// are float32 per 64 pixels, everything across rows, channels of a group and samples is added in double in a fixed order:
// no atomics, the same bits on every run.
//
// Two regimes.
//   split (any shape): k_gn_rows writes [N][ceil(HW/64)][2][C] partial rows (one wave per 64 pixels x 32 channels, folded with
//     cross-lane adds, no LDS) -> k_gn_finalize_* (one workgroup per (sample, group)) writes per-(n, c) coefficient rows ->
//     k_gn_apply_*.  When HW % 64 == 0 the forward can take the rows a convolution's epilogue already wrote (stat_rows) and
//     never reads the map for its statistics.
//   small (HW <= 64 and C <= 512, the RoI tiles): ONE launch, a workgroup owns whole samples: sums, finalize in LDS, apply; the
//     second read of the tile comes from cache.
// Backward of both regimes ends with k_gn_param_grads: the per-(n, c) terms added over samples in double, += into dgamma / dbeta.
//
// Workspace (floats): rows N * rps * 2 * C | coefficients N * 4 * C | parameter-gradient terms N * 2 * C, rps = ceil(HW / 64).
#include "cr_common.h"
#include "cr_elem.h"
#include "cr3dod.h"

namespace {

constexpr int GN_SLICE = 32;            // channels a wave (split regime) covers: C % 32 == 0
constexpr int GN_SMALL_HW = 64;
constexpr int GN_SMALL_C = 512;
constexpr int GN_MAXBLOCKS = 2048;

template <typename T> struct gn_vec { static constexpr int V = 8; };
template <> struct gn_vec<float> { static constexpr int V = 4; };

// sum over the pixel lanes of a wave (lanes that differ in the bits >= TPP): a butterfly, the same order in every lane
template <int TPP> __device__ __forceinline__ float gn_wave_fold(float v) {
#pragma unroll
    for (int off = TPP; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- split regime, pass 1: rows[n][j][2][C] of 64 pixels each.  blockIdx.y = channel slice; a wave takes (n, j) items ---------
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void k_gn_rows(const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ y,
                                                 const float* __restrict__ mean_rstd, float* __restrict__ rows, int N,
                                                 int64_t HW, int C, int G, int rps) {
    constexpr int V = gn_vec<T>::V, TPP = GN_SLICE / V, LPW = 64 / TPP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cv = lane % TPP, pl = lane / TPP;
    const int c0 = blockIdx.y * GN_SLICE + cv * V;
    const int cpg = C / G;
    int gi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) gi[e] = (c0 + e) / cpg;
    const int64_t items = (int64_t)N * rps;
    for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < items; it += (int64_t)gridDim.x * 4) {
        const int n = (int)(it / rps), j = (int)(it - (int64_t)n * rps);
        float mu[V], a[V], b[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            a[e] = 0.f; b[e] = 0.f;
            mu[e] = BWD ? mean_rstd[((size_t)n * G + gi[e]) * 2] : 0.f;
        }
        const int64_t p1 = (int64_t)j * 64 + 64 < HW ? (int64_t)j * 64 + 64 : HW;
        for (int64_t p = (int64_t)j * 64 + pl; p < p1; p += LPW) {
            const size_t i = ((size_t)n * HW + p) * C + c0;
            float xv[V];
            loadv<T, V>(x, i, xv);
            if (BWD) {
                float gv[V];
                loadv<T, V>(dy, i, gv);
                if (y) {
                    float yv[V];
                    loadv<T, V>(y, i, yv);
#pragma unroll
                    for (int e = 0; e < V; ++e) gv[e] = yv[e] > 0.f ? gv[e] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < V; ++e) { a[e] += gv[e]; b[e] += gv[e] * (xv[e] - mu[e]); }
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) { a[e] += xv[e]; b[e] += xv[e] * xv[e]; }
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) { a[e] = gn_wave_fold<TPP>(a[e]); b[e] = gn_wave_fold<TPP>(b[e]); }
        if (pl == 0) {
            float* dst = rows + ((size_t)n * rps + j) * 2 * C + c0;
#pragma unroll
            for (int e = 0; e < V; ++e) { dst[e] = a[e]; dst[C + e] = b[e]; }
        }
    }
}

// 256 doubles -> their sum in every thread's view of s[0] (fixed tree); the whole workgroup calls it
__device__ __forceinline__ void gn_tree2(double* s, double* q) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) { s[t] += s[t + off]; q[t] += q[t + off]; }
        __syncthreads();
    }
}

// ---- split regime, forward finalize: workgroup (n, g) folds rows x channels of its group in double -> mean_rstd, coefficients
// coef[n][0][c] = mu, coef[n][1][c] = gamma_c * r
__global__ __launch_bounds__(256) void k_gn_finalize_fwd(const float* __restrict__ rows, int rps, int64_t HW, int C, int G,
                                                         float eps, const float* __restrict__ gamma,
                                                         float* __restrict__ mean_rstd, float* __restrict__ coef) {
    __shared__ double ss[256], sq[256];
    const int t = threadIdx.x;
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int cpg = C / G;
    const float* base = rows + (size_t)n * rps * 2 * C + (size_t)g * cpg;
    double s = 0.0, q = 0.0;
    const int64_t cnt = (int64_t)rps * cpg;
    for (int64_t e = t; e < cnt; e += 256) {
        const int64_t j = e / cpg;
        const int k = (int)(e - j * cpg);
        s += (double)base[(size_t)j * 2 * C + k];
        q += (double)base[(size_t)j * 2 * C + C + k];
    }
    ss[t] = s; sq[t] = q;
    gn_tree2(ss, sq);
    const double count = (double)HW * (double)cpg;
    const double mean = ss[0] / count;
    double var = sq[0] / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float mf = (float)mean, rf = (float)(1.0 / sqrt(var + (double)eps));
    if (t == 0) {
        mean_rstd[(size_t)blockIdx.x * 2] = mf;
        mean_rstd[(size_t)blockIdx.x * 2 + 1] = rf;
    }
    for (int k = t; k < cpg; k += 256) {
        const int c = g * cpg + k;
        coef[((size_t)n * 4 + 0) * C + c] = mf;
        coef[((size_t)n * 4 + 1) * C + c] = gamma[c] * rf;
    }
}

// ---- split regime, backward finalize: workgroup (n, g).  Channel totals in double (row lanes, then lane order), the group's
// m1 / m2 from them.  coef[n][0..3][c] = mu, gamma_c r, B, D;  terms[n][0][c] = r S_gx, terms[n][1][c] = S_g
__global__ __launch_bounds__(256) void k_gn_finalize_bwd(const float* __restrict__ rows, int rps, int64_t HW, int C, int G,
                                                         const float* __restrict__ gamma, const float* __restrict__ mean_rstd,
                                                         float* __restrict__ coef, float* __restrict__ terms) {
    __shared__ double sa[256], sb[256];
    const int t = threadIdx.x;
    const int n = blockIdx.x / G, g = blockIdx.x - n * G;
    const int cpg = C / G;
    const float mu = mean_rstd[(size_t)blockIdx.x * 2], r = mean_rstd[(size_t)blockIdx.x * 2 + 1];
    const int kch = cpg < 256 ? cpg : 256;              // channels per pass
    const int L = 256 / kch;                            // row lanes per channel
    double m1 = 0.0, m2 = 0.0;                          // (thread 0's are the group's)
    for (int k0 = 0; k0 < cpg; k0 += kch) {
        const int k = t % kch, l = t / kch;
        const bool live = l < L && k0 + k < cpg;
        const int c = g * cpg + k0 + k;
        double a = 0.0, b = 0.0;
        if (live) {
            const float* p = rows + (size_t)n * rps * 2 * C + c;
            for (int j = l; j < rps; j += L) {
                a += (double)p[(size_t)j * 2 * C];
                b += (double)p[(size_t)j * 2 * C + C];
            }
        }
        sa[t] = a; sb[t] = b;
        __syncthreads();
        double u1 = 0.0, u2 = 0.0;
        if (live && l == 0) {
            double ta = 0.0, tb = 0.0;
            for (int i = 0; i < L; ++i) { ta += sa[i * kch + k]; tb += sb[i * kch + k]; }        // fixed order
            const double gx = (double)r * tb;
            terms[((size_t)n * 2 + 0) * C + c] = (float)gx;
            terms[((size_t)n * 2 + 1) * C + c] = (float)ta;
            u1 = (double)gamma[c] * ta;
            u2 = (double)gamma[c] * gx;
        }
        __syncthreads();
        sa[t] = u1; sb[t] = u2;
        gn_tree2(sa, sb);
        m1 += sa[0]; m2 += sb[0];
        __syncthreads();
    }
    const double count = (double)HW * (double)cpg;
    m1 /= count; m2 /= count;
    const float Bf = (float)(-(double)r * (double)r * m2), Df = (float)(-(double)r * m1);
    for (int k = t; k < cpg; k += 256) {
        const int c = g * cpg + k;
        coef[((size_t)n * 4 + 0) * C + c] = mu;
        coef[((size_t)n * 4 + 1) * C + c] = gamma[c] * r;
        coef[((size_t)n * 4 + 2) * C + c] = Bf;
        coef[((size_t)n * 4 + 3) * C + c] = Df;
    }
}

// ---- split regime, pass 3.  blockIdx.y = channel slice, blockIdx.x = (n, pixel chunk): a thread's channels and sample are
// fixed, its coefficients live in registers
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void k_gn_apply(const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ y,
                                                  const float* __restrict__ coef, const float* __restrict__ beta,
                                                  T* __restrict__ out, int64_t HW, int C, int chunks, int64_t px_per_block,
                                                  int relu) {
    constexpr int V = gn_vec<T>::V, TPP = GN_SLICE / V, LANES = 256 / TPP;
    const int t = threadIdx.x, cv = t % TPP, pl = t / TPP;
    const int c0 = blockIdx.y * GN_SLICE + cv * V;
    const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
    float mu[V], sc[V], k2[V], k3[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        mu[e] = coef[((size_t)n * 4 + 0) * C + c0 + e];
        sc[e] = coef[((size_t)n * 4 + 1) * C + c0 + e];
        k2[e] = BWD ? coef[((size_t)n * 4 + 2) * C + c0 + e] : beta[c0 + e];
        k3[e] = BWD ? coef[((size_t)n * 4 + 3) * C + c0 + e] : 0.f;
    }
    const int64_t p0 = (int64_t)chunk * px_per_block, p1 = p0 + px_per_block < HW ? p0 + px_per_block : HW;
    for (int64_t p = p0 + pl; p < p1; p += LANES) {
        const size_t i = ((size_t)n * HW + p) * C + c0;
        float xv[V], o[V];
        loadv<T, V>(x, i, xv);
        if (BWD) {
            float gv[V];
            loadv<T, V>(dy, i, gv);
            if (y) {
                float yv[V];
                loadv<T, V>(y, i, yv);
#pragma unroll
                for (int e = 0; e < V; ++e) gv[e] = yv[e] > 0.f ? gv[e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = sc[e] * gv[e] + (k2[e] * (xv[e] - mu[e]) + k3[e]);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float v = (xv[e] - mu[e]) * sc[e] + k2[e];
                o[e] = relu ? fmaxf(v, 0.f) : v;
            }
        }
        storev<T, V>(out, i, o);
    }
}

// ---- small regime: HW <= 64, C <= 512.  A workgroup owns whole samples (n = blockIdx.x, + gridDim.x, ...).  Thread (pixel
// lane pl, channel vector cv) keeps its channels for the whole kernel.  LDS: buf = the pixel lanes' partial sums ([lanes][C],
// lanes * C <= 256 * V <= 2048), later the sample's coefficient rows ([4][512]); chs = channel totals.
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void k_gn_small(const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ y,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ mean_rstd, float* __restrict__ terms,
                                                  T* __restrict__ out, int N, int HW, int C, int G, float eps, int relu) {
    constexpr int V = gn_vec<T>::V;
    __shared__ float buf[2048];
    __shared__ float chs[2][GN_SMALL_C];
    const int t = threadIdx.x;
    const int cg = C / V;                               // <= 128
    const int lanes = 256 / cg;
    const bool active = t < lanes * cg;
    const int cv = t % cg, pl = t / cg, c0 = cv * V;
    const int cpg = C / G;
    const double count = (double)HW * (double)cpg;
    int gi[V];
    float be[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        gi[e] = (c0 + e) / cpg;
        be[e] = BWD ? 0.f : beta[c0 + e];
    }
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const size_t base = (size_t)n * HW * C + c0;
        float mu[V], a[V], b[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            a[e] = 0.f; b[e] = 0.f;
            mu[e] = BWD ? mean_rstd[((size_t)n * G + gi[e]) * 2] : 0.f;
        }
        if (active) {
            for (int p = pl; p < HW; p += lanes) {
                const size_t i = base + (size_t)p * C;
                float xv[V];
                loadv<T, V>(x, i, xv);
                if (BWD) {
                    float gv[V];
                    loadv<T, V>(dy, i, gv);
                    if (y) {
                        float yv[V];
                        loadv<T, V>(y, i, yv);
#pragma unroll
                        for (int e = 0; e < V; ++e) gv[e] = yv[e] > 0.f ? gv[e] : 0.f;
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) { a[e] += gv[e]; b[e] += gv[e] * (xv[e] - mu[e]); }
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) { a[e] += xv[e]; b[e] += xv[e] * xv[e]; }
                }
            }
        }
        // channel totals: the pixel lanes of a channel in lane order, in double
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            if (active) {
#pragma unroll
                for (int e = 0; e < V; ++e) buf[pl * C + c0 + e] = which ? b[e] : a[e];
            }
            __syncthreads();
            for (int c = t; c < C; c += 256) {
                double s = 0.0;
                for (int l = 0; l < lanes; ++l) s += (double)buf[l * C + c];
                chs[which][c] = (float)s;
                if (BWD) {
                    const float r = mean_rstd[((size_t)n * G + c / cpg) * 2 + 1];
                    terms[((size_t)n * 2 + (which ? 0 : 1)) * C + c] = which ? (float)((double)r * s) : (float)s;
                }
            }
            __syncthreads();
        }
        // groups: one thread each; coefficient rows of the sample into buf
        for (int g = t; g < G; g += 256) {
            double s = 0.0, q = 0.0;
            if (BWD) {
                const float muf = mean_rstd[((size_t)n * G + g) * 2], r = mean_rstd[((size_t)n * G + g) * 2 + 1];
                for (int k = 0; k < cpg; ++k) {
                    const int c = g * cpg + k;
                    s += (double)gamma[c] * (double)chs[0][c];
                    q += (double)gamma[c] * (double)chs[1][c];
                }
                const double m1 = s / count, m2 = (double)r * q / count;
                const float Bf = (float)(-(double)r * (double)r * m2), Df = (float)(-(double)r * m1);
                for (int k = 0; k < cpg; ++k) {
                    const int c = g * cpg + k;
                    buf[c] = muf;
                    buf[GN_SMALL_C + c] = gamma[c] * r;
                    buf[2 * GN_SMALL_C + c] = Bf;
                    buf[3 * GN_SMALL_C + c] = Df;
                }
            } else {
                for (int k = 0; k < cpg; ++k) {
                    s += (double)chs[0][g * cpg + k];
                    q += (double)chs[1][g * cpg + k];
                }
                const double mean = s / count;
                double var = q / count - mean * mean;
                if (var < 0.0) var = 0.0;
                const float mf = (float)mean, rf = (float)(1.0 / sqrt(var + (double)eps));
                mean_rstd[((size_t)n * G + g) * 2] = mf;
                mean_rstd[((size_t)n * G + g) * 2 + 1] = rf;
                for (int k = 0; k < cpg; ++k) {
                    const int c = g * cpg + k;
                    buf[c] = mf;
                    buf[GN_SMALL_C + c] = gamma[c] * rf;
                }
            }
        }
        __syncthreads();
        if (active) {
            float cm[V], sc[V], k2[V], k3[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                cm[e] = buf[c0 + e];
                sc[e] = buf[GN_SMALL_C + c0 + e];
                k2[e] = BWD ? buf[2 * GN_SMALL_C + c0 + e] : be[e];
                k3[e] = BWD ? buf[3 * GN_SMALL_C + c0 + e] : 0.f;
            }
            for (int p = pl; p < HW; p += lanes) {                 // the tile again, from cache
                const size_t i = base + (size_t)p * C;
                float xv[V], o[V];
                loadv<T, V>(x, i, xv);
                if (BWD) {
                    float gv[V];
                    loadv<T, V>(dy, i, gv);
                    if (y) {
                        float yv[V];
                        loadv<T, V>(y, i, yv);
#pragma unroll
                        for (int e = 0; e < V; ++e) gv[e] = yv[e] > 0.f ? gv[e] : 0.f;
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] = sc[e] * gv[e] + (k2[e] * (xv[e] - cm[e]) + k3[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float v = (xv[e] - cm[e]) * sc[e] + k2[e];
                        o[e] = relu ? fmaxf(v, 0.f) : v;
                    }
                }
                storev<T, V>(out, i, o);
            }
        }
        __syncthreads();                                           // buf is rewritten by the next sample
    }
}

// ---- dgamma[c] += sum_n terms[n][0][c], dbeta[c] += sum_n terms[n][1][c]: 16 sample lanes per channel in double, then lane order
__global__ __launch_bounds__(512) void k_gn_param_grads(const float* __restrict__ terms, int N, int C,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sd[2][16][32];
    const int t = threadIdx.x, ch = t & 31, rl = t >> 5;
    const int c = blockIdx.x * 32 + ch;
    double s = 0.0, q = 0.0;
    for (int n = rl; n < N; n += 16) {
        s += (double)terms[((size_t)n * 2 + 0) * C + c];
        q += (double)terms[((size_t)n * 2 + 1) * C + c];
    }
    sd[0][rl][ch] = s; sd[1][rl][ch] = q;
    __syncthreads();
    if (t < 64) {
        const int which = t >> 5;
        double tot = 0.0;
        for (int r = 0; r < 16; ++r) tot += sd[which][r][ch];      // fixed order
        float* dst = which ? dbeta : dgamma;
        dst[c] += (float)tot;
    }
}

inline int gn_rps(int64_t HW) { return (int)cr_cdiv(HW, 64); }

int64_t gn_ws_floats(int64_t N, int64_t HW, int C) { return N * C * (2 * (int64_t)gn_rps(HW) + 6); }

bool gn_small(int64_t HW, int C) { return HW <= GN_SMALL_HW && C <= GN_SMALL_C; }

bool gn_domain(int64_t N, int64_t HW, int C) {
    return N >= 1 && N <= (1 << 24) && HW >= 1 && HW <= ((int64_t)1 << 31) && C >= 32 && C % 32 == 0 && C <= 2048;
}

bool gn_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int gn_check(const char* who, int64_t N, int64_t HW, int C, int G, int relu, int act_f32, const float* ws, int64_t ws_floats) {
    CR_CHECK_ARG(gn_domain(N, HW, C), "%s: unsupported shape N=%lld HW=%lld C=%d (C %% 32 == 0, 32 <= C <= 2048, N, HW >= 1)", who,
                 (long long)N, (long long)HW, C);
    CR_CHECK_ARG(G >= 1 && C % G == 0, "%s: G=%d does not divide C=%d", who, G, C);
    CR_CHECK_ARG(relu == 0 || relu == 1, "%s: relu must be 0 or 1 (got %d)", who, relu);
    CR_CHECK_ARG(act_f32 >= 0 && act_f32 <= 2, "%s: act_f32 must be 0, 1 or 2 (got %d)", who, act_f32);
    CR_CHECK_ARG(gn_aligned(ws, 16), "%s: the workspace must be 16-byte aligned", who);
    const int64_t need = gn_ws_floats(N, HW, C);
    CR_CHECK_ARG(ws_floats >= need, "%s: workspace of %lld floats, %lld needed (cr_groupnorm_ws_floats)", who,
                 (long long)ws_floats, (long long)need);
    return CR_OK;
}

// grid of k_gn_rows: 4 waves per workgroup, one (n, row) item per wave and turn
dim3 gn_rows_grid(int64_t N, int rps, int C) {
    const int slices = C / GN_SLICE;
    int64_t bx = cr_cdiv(N * rps, 4), cap = GN_MAXBLOCKS / slices;
    if (cap < 1) cap = 1;
    if (bx > cap) bx = cap;
    return dim3((unsigned)bx, (unsigned)slices);
}

template <typename T>
void gn_apply_plan(int64_t N, int64_t HW, int C, int& chunks, int64_t& ppb) {
    constexpr int LANES = 256 / (GN_SLICE / gn_vec<T>::V);
    const int64_t slices = C / GN_SLICE;
    int64_t ch = GN_MAXBLOCKS / (N * slices);
    const int64_t most = cr_cdiv(HW, LANES);
    if (ch > most) ch = most;
    if (ch < 1) ch = 1;
    ppb = cr_cdiv(HW, ch);
    chunks = (int)cr_cdiv(HW, ppb);
}

template <typename T>
int gn_fwd_launch(cr_ctx* ctx, const T* x, const float* gamma, const float* beta, const float* stat_rows, T* y,
                  float* mean_rstd, float* ws, int N, int64_t HW, int C, int G, float eps, int relu) {
    if (gn_small(HW, C) && !stat_rows) {
        const unsigned grid = (unsigned)(N < 1024 ? N : 1024);
        hipLaunchKernelGGL((k_gn_small<T, false>), dim3(grid), dim3(256), 0, ctx->stream, x, (const T*)nullptr, (const T*)nullptr,
                           gamma, beta, mean_rstd, (float*)nullptr, y, N, (int)HW, C, G, eps, relu);
        CR_LAUNCH_CHECK();
        return CR_OK;
    }
    const int rps = gn_rps(HW);
    float* rows = ws;
    float* coef = ws + (size_t)N * rps * 2 * C;
    if (!stat_rows) {
        hipLaunchKernelGGL((k_gn_rows<T, false>), gn_rows_grid(N, rps, C), dim3(256), 0, ctx->stream, x, (const T*)nullptr,
                           (const T*)nullptr, (const float*)nullptr, rows, N, HW, C, G, rps);
        CR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_gn_finalize_fwd, dim3((unsigned)(N * G)), dim3(256), 0, ctx->stream, stat_rows ? stat_rows : rows, rps,
                       HW, C, G, eps, gamma, mean_rstd, coef);
    CR_LAUNCH_CHECK();
    int chunks; int64_t ppb;
    gn_apply_plan<T>(N, HW, C, chunks, ppb);
    hipLaunchKernelGGL((k_gn_apply<T, false>), dim3((unsigned)(N * chunks), (unsigned)(C / GN_SLICE)), dim3(256), 0, ctx->stream,
                       x, (const T*)nullptr, (const T*)nullptr, coef, beta, y, HW, C, chunks, ppb, relu);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

template <typename T>
int gn_bwd_launch(cr_ctx* ctx, const T* dy, const T* x, const T* y, const float* mean_rstd, const float* gamma, float* ws,
                  T* dx, float* dgamma, float* dbeta, int N, int64_t HW, int C, int G) {
    const int rps = gn_rps(HW);
    float* rows = ws;
    float* coef = ws + (size_t)N * rps * 2 * C;
    float* terms = coef + (size_t)N * 4 * C;
    if (gn_small(HW, C)) {
        const unsigned grid = (unsigned)(N < 1024 ? N : 1024);
        hipLaunchKernelGGL((k_gn_small<T, true>), dim3(grid), dim3(256), 0, ctx->stream, x, dy, y, gamma, (const float*)nullptr,
                           const_cast<float*>(mean_rstd), terms, dx, N, (int)HW, C, G, 0.f, 0);
        CR_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL((k_gn_rows<T, true>), gn_rows_grid(N, rps, C), dim3(256), 0, ctx->stream, x, dy, y, mean_rstd, rows, N,
                           HW, C, G, rps);
        CR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_gn_finalize_bwd, dim3((unsigned)(N * G)), dim3(256), 0, ctx->stream, rows, rps, HW, C, G, gamma,
                           mean_rstd, coef, terms);
        CR_LAUNCH_CHECK();
        int chunks; int64_t ppb;
        gn_apply_plan<T>(N, HW, C, chunks, ppb);
        hipLaunchKernelGGL((k_gn_apply<T, true>), dim3((unsigned)(N * chunks), (unsigned)(C / GN_SLICE)), dim3(256), 0,
                           ctx->stream, x, dy, y, coef, (const float*)nullptr, dx, HW, C, chunks, ppb, 0);
        CR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_gn_param_grads, dim3((unsigned)(C / 32)), dim3(512), 0, ctx->stream, terms, N, C, dgamma, dbeta);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

}  // namespace

extern "C" int cr_groupnorm_ws_floats(int64_t N, int64_t HW, int C) {
    if (!gn_domain(N, HW, C)) return 0;
    const int64_t n = gn_ws_floats(N, HW, C);
    return n > 0x7fffffff ? 0 : (int)n;
}

extern "C" int cr_groupnorm_fwd(cr_ctx* ctx, const void* x, const float* gamma, const float* beta, const float* stat_rows,
                                void* y, float* mean_rstd, float* ws, int64_t ws_floats, int N, int64_t HW, int C, int G,
                                float eps, int relu, int act_f32) {
    CR_CHECK_ARG(ctx && x && gamma && beta && y && mean_rstd && ws, "cr_groupnorm_fwd: NULL pointer");
    if (int rc = gn_check("cr_groupnorm_fwd", N, HW, C, G, relu, act_f32, ws, ws_floats)) return rc;
    CR_CHECK_ARG(eps >= 0.f, "cr_groupnorm_fwd: eps must be >= 0 (got %g)", (double)eps);
    CR_CHECK_ARG(gn_aligned(x, 16) && gn_aligned(y, 16), "cr_groupnorm_fwd: x and y must be 16-byte aligned");
    CR_CHECK_ARG(gn_aligned(gamma, 4) && gn_aligned(beta, 4) && gn_aligned(mean_rstd, 4) && gn_aligned(stat_rows, 4),
                 "cr_groupnorm_fwd: misaligned float buffer");
    CR_CHECK_ARG(!stat_rows || HW % 64 == 0, "cr_groupnorm_fwd: stat_rows need HW %% 64 == 0 (got HW=%lld): a row of 64 pixels "
                 "would straddle two samples", (long long)HW);
    if (act_f32)
        return gn_fwd_launch<float>(ctx, (const float*)x, gamma, beta, stat_rows, (float*)y, mean_rstd, ws, N, HW, C, G, eps, relu);
    return gn_fwd_launch<u16>(ctx, (const u16*)x, gamma, beta, stat_rows, (u16*)y, mean_rstd, ws, N, HW, C, G, eps, relu);
}

extern "C" int cr_groupnorm_bwd(cr_ctx* ctx, const void* dy, const void* x, const void* y, const float* mean_rstd,
                                const float* gamma, float* ws, int64_t ws_floats, void* dx, float* dgamma, float* dbeta, int N,
                                int64_t HW, int C, int G, int relu, int act_f32) {
    CR_CHECK_ARG(ctx && dy && x && mean_rstd && gamma && ws && dx && dgamma && dbeta, "cr_groupnorm_bwd: NULL pointer");
    if (int rc = gn_check("cr_groupnorm_bwd", N, HW, C, G, relu, act_f32, ws, ws_floats)) return rc;
    CR_CHECK_ARG(!relu || y, "cr_groupnorm_bwd: relu needs the stored output y (the mask is y > 0)");
    CR_CHECK_ARG(gn_aligned(dy, 16) && gn_aligned(x, 16) && gn_aligned(y, 16) && gn_aligned(dx, 16),
                 "cr_groupnorm_bwd: dy, x, y and dx must be 16-byte aligned");
    CR_CHECK_ARG(gn_aligned(gamma, 4) && gn_aligned(mean_rstd, 4) && gn_aligned(dgamma, 4) && gn_aligned(dbeta, 4),
                 "cr_groupnorm_bwd: misaligned float buffer");
    CR_CHECK_ARG(dgamma != dbeta, "cr_groupnorm_bwd: dgamma and dbeta must be separate buffers");
    const void* mask = relu ? y : nullptr;
    if (act_f32)
        return gn_bwd_launch<float>(ctx, (const float*)dy, (const float*)x, (const float*)mask, mean_rstd, gamma, ws, (float*)dx,
                                    dgamma, dbeta, N, HW, C, G);
    return gn_bwd_launch<u16>(ctx, (const u16*)dy, (const u16*)x, (const u16*)mask, mean_rstd, gamma, ws, (u16*)dx, dgamma,
                              dbeta, N, HW, C, G);
}
