// Backward kernels of the Depth-Anything-V2 training step (fine-tuning for metric depth; reference:
// depth/metric_depth/train.py with util/loss.py and util/metric.py): attention, LayerNorm, GELU, LayerScale + residual and
// the align_corners bilinear resize, plus the masked depth reduction behind the SiLog loss and the nine validation metrics.
// Activations and activation gradients are bf16 (the training route's residual stream float32), every accumulation is float32 (float64 for the depth sums), parameter
// gradients are float32.  Nothing here uses a float atomic: every sum has one owner and a fixed order, so two runs of the
// same step give the same bits.
#include "cr_common.h"
#include <math.h>
#include <stdlib.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

__device__ __forceinline__ float wbf2f(u16 b) { return __uint_as_float(((unsigned)b) << 16); }
__device__ __forceinline__ u16 wf2bf(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(u16, b);
}
__device__ __forceinline__ void unpack8(const uint4 u, float* v) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = wbf2f((u16)(w[e] & 0xffff));
        v[2 * e + 1] = wbf2f((u16)(w[e] >> 16));
    }
}
__device__ __forceinline__ uint4 pack8(const float* v) {
    unsigned o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (unsigned)wf2bf(v[2 * e]) | ((unsigned)wf2bf(v[2 * e + 1]) << 16);
    return make_uint4(o[0], o[1], o[2], o[3]);
}

static inline unsigned grid_1d(int64_t work, int per_block, int cap) {
    const int64_t b = cr_cdiv(work, per_block);
    return (unsigned)(b < cap ? b : cap);
}

// ---------------------------------------------------------------------------------------------------------------------
// Attention backward, head_dim 64, on the packed qkv of the forward (vit.hip: k_attention_fwd, whose LSE variant wrote
// lse = log sum_k exp(scale q.k) per query).  With P = exp(scale q.k - lse), dP = dO V^T and delta = rowsum(P o dP):
//     dV = P^T dO,   dS = P o (dP - delta),   dQ = scale dS K,   dK = scale dS^T Q.
// delta equals rowsum(dO o O), but O exists only rounded to bf16: where one key dominates a row, dP - delta cancels and the
// 2^-9 of that rounding is as large as dS itself (measured on the peaked test case: dq off by 5.9e-3 normwise against
// 2.4e-3 for the roundings of P and dS alone).  So delta is summed from the float32 P and dP in a pass of its own.
// Three launches of one kernel template, each owning its outputs (no sum across workgroups):
//   * MODE 2: a wave OWNS 16 queries and streams the keys -> delta (S and dP only);
//   * MODE 0: the same ownership -> dQ;
//   * MODE 1: a wave OWNS 16 keys and streams the queries  -> dK and dV.
// The MFMA orientation is the forward's: the streamed rows ("other") are the A operand, the owned rows the B operand, so a
// lane's 16 results of S^T / dP^T all belong to ONE owned row (column lane & 15) and are, after rounding to bf16, already
// the B operand of the products that sum over the streamed index (k index of the MFMA mapped to streamed rows as in the
// forward: kk = 8g+j -> row 32s + 16(j/4) + 4g + (j%4)).  Those products need the streamed tile transposed ([d][row]) as
// their A operand: every tile is written to LDS twice, row-major for S / dP and transposed (with the forward's column
// swizzle) for the accumulating products.  P and dS are rounded to bf16 once, dq / dk / dv once at the store.
// ---------------------------------------------------------------------------------------------------------------------
#define AB_D 64
#define AB_T 64
#define AB_PAD 8

template <int MODE, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_attention_bwd(const u16* __restrict__ qkv, const u16* __restrict__ dout,
                                                              const float* __restrict__ lse, float* __restrict__ delta,
                                                              u16* __restrict__ dqkv, int B, int N, int H, float scale,
                                                              int otiles) {
    constexpr bool KV = MODE == 1, DELTA = MODE == 2;
    constexpr int T = 64 * WAVES, NCH = 512 / T;
    __shared__ __attribute__((aligned(16))) u16 sA[AB_T][AB_D + AB_PAD];       // streamed rows of K (dQ pass) / Q (dK,dV pass)
    __shared__ __attribute__((aligned(16))) u16 sB[AB_T][AB_D + AB_PAD];       // streamed rows of V / dO
    __shared__ __attribute__((aligned(16))) u16 sAt[DELTA ? 1 : AB_D][AB_T + AB_PAD];      // the same tiles, [d][row]
    __shared__ __attribute__((aligned(16))) u16 sBt[KV ? AB_D : 1][AB_T + AB_PAD];
    __shared__ float sL[AB_T], sDl[AB_T];                                      // lse / delta of streamed queries (KV pass)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int bh = (int)blockIdx.x / otiles, ot = (int)blockIdx.x - bh * otiles;
    const int b = bh / H, h = bh - b * H;
    const int own = ot * 16 * WAVES + wave * 16 + c;          // this lane's owned row (query or key)
    const bool own_ok = own < N;
    const size_t rs = (size_t)3 * H * AB_D, os = (size_t)H * AB_D;
    const u16* Qb = qkv + (size_t)b * N * rs + (size_t)h * AB_D;
    const u16* Kb = Qb + (size_t)H * AB_D;
    const u16* Vb = Qb + (size_t)2 * H * AB_D;
    const u16* dOb = dout + (size_t)b * N * os + (size_t)h * AB_D;
    const float* lse_b = lse + ((size_t)b * H + h) * N;
    float* del_b = delta + ((size_t)b * H + h) * N;
    // owned fragments (B operands): row `own`, d = 32 s + 8 g .. + 7
    const u16* ownA = KV ? Kb : Qb;
    const u16* ownB = KV ? Vb : dOb;
    const size_t ownBs = KV ? rs : os;
    const u16* othA = KV ? Qb : Kb;
    const u16* othB = KV ? dOb : Vb;
    const size_t othBs = KV ? os : rs;
    bf16x8 oa[2], ob[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        uint4 va = make_uint4(0, 0, 0, 0), vb = make_uint4(0, 0, 0, 0);
        if (own_ok) {
            va = *reinterpret_cast<const uint4*>(ownA + (size_t)own * rs + 32 * s + 8 * g);
            vb = *reinterpret_cast<const uint4*>(ownB + (size_t)own * ownBs + 32 * s + 8 * g);
        }
        oa[s] = __builtin_bit_cast(bf16x8, va);
        ob[s] = __builtin_bit_cast(bf16x8, vb);
    }
    float own_lse = 0.f, own_del = 0.f;
    if (!KV && own_ok) {
        own_lse = lse_b[own];
        if (!DELTA) own_del = del_b[own];
    }
    float dsum = 0.f;                        // MODE 2: this lane's share of delta[own]
    f32x4 acc0[4], acc1[4];                  // dQ^T (dQ pass) / dK^T and dV^T (KV pass): rows d = 16 db + 4 g + e, column c
#pragma unroll
    for (int i = 0; i < 4; ++i) acc0[i] = acc1[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int ntiles = (N + AB_T - 1) / AB_T;
    uint4 ra[NCH], rb[NCH];
    float rl = 0.f, rd = 0.f;
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + T * i;
            const int row = t * AB_T + (idx >> 3), d8 = (idx & 7) * 8;
            ra[i] = make_uint4(0, 0, 0, 0);
            rb[i] = make_uint4(0, 0, 0, 0);
            if (row < N) {
                ra[i] = *reinterpret_cast<const uint4*>(othA + (size_t)row * rs + d8);
                rb[i] = *reinterpret_cast<const uint4*>(othB + (size_t)row * othBs + d8);
            }
        }
        if (KV && tid < AB_T) {
            const int row = t * AB_T + tid;
            rl = row < N ? lse_b[row] : 0.f;
            rd = row < N ? del_b[row] : 0.f;
        }
    };
    auto store_t = [&](u16 (*dst)[AB_T + AB_PAD], const uint4 v, int row, int d8) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        const int rx = row ^ (((d8 >> 3) & 7) << 3);            // the forward's bank swizzle of the transposed image
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dst[d8 + 2 * e][rx] = (u16)(w[e] & 0xffff);
            dst[d8 + 2 * e + 1][rx] = (u16)(w[e] >> 16);
        }
    };
    load_tile(0);
    for (int t = 0; t < ntiles; ++t) {
        const int r0 = t * AB_T;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + T * i;
            const int row = idx >> 3, d8 = (idx & 7) * 8;
            *reinterpret_cast<uint4*>(&sA[row][d8]) = ra[i];
            *reinterpret_cast<uint4*>(&sB[row][d8]) = rb[i];
            if (!DELTA) store_t(sAt, ra[i], row, d8);
            if (KV) store_t(sBt, rb[i], row, d8);
        }
        if (KV && tid < AB_T) {
            sL[tid] = rl;
            sDl[tid] = rd;
        }
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t + 1);

        // S^T and dP^T: rows = streamed 16 rb + 4 g + e, column = owned row c
        f32x4 s4[4], dp[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            s4[kb] = dp[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 fa = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&sA[16 * kb + c][32 * s + 8 * g]));
                const bf16x8 fb = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(&sB[16 * kb + c][32 * s + 8 * g]));
                s4[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, oa[s], s4[kb], 0, 0, 0);
                dp[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, ob[s], dp[kb], 0, 0, 0);
            }
        }
        unsigned pP[4][2], pS[4][2];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            float p[4], ds[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int lr = 16 * kb + 4 * g + e;
                const bool ok = own_ok && (r0 + lr < N);
                const float l = KV ? sL[lr] : own_lse, dl = KV ? sDl[lr] : own_del;
                p[e] = ok ? __expf(s4[kb][e] * scale - l) : 0.f;
                ds[e] = p[e] * (dp[kb][e] - dl);
                if (DELTA) dsum += p[e] * dp[kb][e];
            }
            pP[kb][0] = (unsigned)wf2bf(p[0]) | ((unsigned)wf2bf(p[1]) << 16);
            pP[kb][1] = (unsigned)wf2bf(p[2]) | ((unsigned)wf2bf(p[3]) << 16);
            pS[kb][0] = (unsigned)wf2bf(ds[0]) | ((unsigned)wf2bf(ds[1]) << 16);
            pS[kb][1] = (unsigned)wf2bf(ds[2]) | ((unsigned)wf2bf(ds[3]) << 16);
        }
        if (DELTA) continue;
        // acc^T[d, own] += sum_rows tile^T[d, row] * (dS | P)^T[row, own]; step s covers row blocks 2s and 2s+1
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 dsf = __builtin_bit_cast(bf16x8, make_uint4(pS[2 * s][0], pS[2 * s][1], pS[2 * s + 1][0], pS[2 * s + 1][1]));
            const bf16x8 pf = __builtin_bit_cast(bf16x8, make_uint4(pP[2 * s][0], pP[2 * s][1], pP[2 * s + 1][0], pP[2 * s + 1][1]));
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const int sw = ((2 * db + (c >> 3)) & 7) << 3;
                const uint2 a0 = *reinterpret_cast<const uint2*>(&sAt[16 * db + c][(32 * s + 4 * g) ^ sw]);
                const uint2 a1 = *reinterpret_cast<const uint2*>(&sAt[16 * db + c][(32 * s + 16 + 4 * g) ^ sw]);
                const bf16x8 fa = __builtin_bit_cast(bf16x8, make_uint4(a0.x, a0.y, a1.x, a1.y));
                acc0[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, dsf, acc0[db], 0, 0, 0);
                if (KV) {
                    const uint2 b0 = *reinterpret_cast<const uint2*>(&sBt[16 * db + c][(32 * s + 4 * g) ^ sw]);
                    const uint2 b1 = *reinterpret_cast<const uint2*>(&sBt[16 * db + c][(32 * s + 16 + 4 * g) ^ sw]);
                    const bf16x8 fb = __builtin_bit_cast(bf16x8, make_uint4(b0.x, b0.y, b1.x, b1.y));
                    acc1[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, pf, acc1[db], 0, 0, 0);
                }
            }
        }
    }
    if (DELTA) {
        dsum += __shfl_xor(dsum, 16, 64);      // the four lanes l, l^16, l^32, l^48 share a query
        dsum += __shfl_xor(dsum, 32, 64);
        if (own_ok && g == 0) del_b[own] = dsum;
        return;
    }
    if (own_ok) {
        u16* dst = dqkv + ((size_t)b * N + own) * rs + (size_t)h * AB_D + (KV ? (size_t)H * AB_D : 0);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            uint2 pk;
            pk.x = (unsigned)wf2bf(acc0[db][0] * scale) | ((unsigned)wf2bf(acc0[db][1] * scale) << 16);
            pk.y = (unsigned)wf2bf(acc0[db][2] * scale) | ((unsigned)wf2bf(acc0[db][3] * scale) << 16);
            *reinterpret_cast<uint2*>(dst + 16 * db + 4 * g) = pk;
            if (KV) {
                pk.x = (unsigned)wf2bf(acc1[db][0]) | ((unsigned)wf2bf(acc1[db][1]) << 16);
                pk.y = (unsigned)wf2bf(acc1[db][2]) | ((unsigned)wf2bf(acc1[db][3]) << 16);
                *reinterpret_cast<uint2*>(dst + (size_t)H * AB_D + 16 * db + 4 * g) = pk;
            }
        }
    }
}

extern "C" int cr_attention_bwd(cr_ctx* ctx, const void* qkv, const void* dout, const float* lse, float* delta, void* dqkv, int B,
                                int N, int H, int D, float scale) {
    CR_CHECK_ARG(ctx && B >= 0 && N >= 0 && H > 0, "cr_attention_bwd: bad args");
    CR_CHECK_ARG(D == AB_D, "cr_attention_bwd: head dimension %d is not built (64 only)", D);
    if ((int64_t)B * N == 0) return CR_OK;
    CR_CHECK_ARG(qkv && dout && lse && delta && dqkv, "cr_attention_bwd: NULL pointer");
    constexpr int WAVES = 4;
    const int otiles = (int)cr_cdiv(N, 16 * WAVES);
    CR_CHECK_ARG((int64_t)B * H * otiles < (1ll << 31), "cr_attention_bwd: grid too large");
    const dim3 grid((unsigned)(B * H * otiles));
#define AB_LAUNCH(MODE_)                                                                                                   \
    hipLaunchKernelGGL((k_attention_bwd<MODE_, WAVES>), grid, dim3(64 * WAVES), 0, ctx->stream, (const u16*)qkv, (const u16*)dout, \
                       lse, delta, (u16*)dqkv, B, N, H, scale, otiles);                                                    \
    CR_LAUNCH_CHECK()
    AB_LAUNCH(2);
    AB_LAUNCH(0);
    AB_LAUNCH(1);
#undef AB_LAUNCH
    return CR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Order-fixed column reduction, second stage: out[j] (+)= sum_p part[p][j] for p = 0 .. P-1 in that order.  The K columns
// are split between two destinations (K0 to out0, the rest to out1): dgamma and dbeta of a LayerNorm, or one vector.
// ---------------------------------------------------------------------------------------------------------------------
#define RED_PARTS 128            // the first stages write at most this many partial rows

__global__ __launch_bounds__(256) void k_colsum_parts(const float* __restrict__ part, int P, int K, int K0, float* __restrict__ out0,
                                                      float* __restrict__ out1, int accumulate) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += part[(size_t)p * K + j];
    float* base = j < K0 ? out0 : out1;              // either destination may be absent: test it BEFORE offsetting
    if (!base) return;
    float* dst = base + (j < K0 ? j : j - K0);
    *dst = accumulate ? *dst + s : s;
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm backward.  One wave per row like the forward (which it repeats for the statistics, so x^ is the forward's):
//   g = dy * gamma,  dx = inv * (g - mean(g) - x^ * mean(g x^)),  dgamma = sum_rows dy x^,  dbeta = sum_rows dy.
// A workgroup walks rows blk*4 + wave + i * 4 * gridDim.x, every lane keeps the partial sums of its own columns in
// registers, the four waves add theirs in wave order through LDS, and the workgroup writes one row of `part`
// (nblk, 2C); k_colsum_parts finishes.
// ---------------------------------------------------------------------------------------------------------------------
// 8 consecutive values of a row that is bf16 (XF32 = false) or float32 (the training route's residual stream)
template <bool XF32>
__device__ __forceinline__ void load_row8(const void* row, int i, float* v) {
    if constexpr (XF32) {
        const float4 a = *reinterpret_cast<const float4*>((const float*)row + i), b = *reinterpret_cast<const float4*>((const float*)row + i + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        unpack8(*reinterpret_cast<const uint4*>((const u16*)row + i), v);
    }
}

// dx is stored in x's type: bf16, or float32 for the float32 residual stream (no cast kernel after it)
template <int NCH, bool XF32>
__global__ __launch_bounds__(256) void k_layernorm_bwd(const void* __restrict__ x, const u16* __restrict__ dy,
                                                       const float* __restrict__ gamma, void* __restrict__ dx,
                                                       float* __restrict__ part, int64_t M, int C, float eps) {
    __shared__ float sred[2][512 * NCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float gam[NCH][8], pg[NCH][8], pb[NCH][8];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int i = lane * 8 + 512 * k;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            gam[k][e] = i < C ? gamma[i + e] : 0.f;
            pg[k][e] = pb[k][e] = 0.f;
        }
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
        const void* xr = XF32 ? (const void*)((const float*)x + row * C) : (const void*)((const u16*)x + row * C);
        const u16* dr = dy + row * C;
        float v[NCH][8], d[NCH][8];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int i = lane * 8 + 512 * k;
            if (i < C) {
                load_row8<XF32>(xr, i, v[k]);
                unpack8(*reinterpret_cast<const uint4*>(dr + i), d[k]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[k][e] = d[k][e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) s += v[k][2 * e] + v[k][2 * e + 1];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const float mean = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            if (lane * 8 + 512 * k < C) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a = v[k][e] - mean;
                    q += a * a;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
        const float inv = rsqrtf(q / (float)C + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const bool in = lane * 8 + 512 * k < C;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = in ? (v[k][e] - mean) * inv : 0.f;
                v[k][e] = xh;
                const float gg = d[k][e] * gam[k][e];
                s1 += gg;
                s2 += gg * xh;
                pg[k][e] += d[k][e] * xh;
                pb[k][e] += d[k][e];
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s1 += __shfl_xor(s1, off, 64);
            s2 += __shfl_xor(s2, off, 64);
        }
        const float m1 = s1 / (float)C, m2 = s2 / (float)C;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int i = lane * 8 + 512 * k;
            if (i < C) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = inv * (d[k][e] * gam[k][e] - m1 - v[k][e] * m2);
                if constexpr (XF32) {
                    float* xo = (float*)dx + row * C + i;
                    *reinterpret_cast<float4*>(xo) = make_float4(o[0], o[1], o[2], o[3]);
                    *reinterpret_cast<float4*>(xo + 4) = make_float4(o[4], o[5], o[6], o[7]);
                } else {
                    *reinterpret_cast<uint4*>((u16*)dx + row * C + i) = pack8(o);
                }
            }
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int k = 0; k < NCH; ++k)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int i = lane * 8 + 512 * k + e;
                    sred[0][i] = w == 0 ? pg[k][e] : sred[0][i] + pg[k][e];
                    sred[1][i] = w == 0 ? pb[k][e] : sred[1][i] + pb[k][e];
                }
        }
        __syncthreads();
    }
    float* pr = part + (size_t)blockIdx.x * 2 * C;
    for (int i = threadIdx.x; i < C; i += 256) {
        pr[i] = sred[0][i];
        pr[C + i] = sred[1][i];
    }
}

extern "C" int cr_layernorm_bwd(cr_ctx* ctx, const void* x, const void* dy, const float* gamma, void* dx, float* dgamma,
                                float* dbeta, float* part, int64_t M, int C, float eps, int accumulate, int x_f32) {
    CR_CHECK_ARG(ctx && M >= 0 && C > 0 && C % 8 == 0, "cr_layernorm_bwd: bad dims M=%lld C=%d", (long long)M, C);
    CR_CHECK_ARG(C <= 2048, "cr_layernorm_bwd: C=%d > 2048 is not built", C);
    if (M == 0) return CR_OK;
    CR_CHECK_ARG(x && dy && gamma && dx && part, "cr_layernorm_bwd: NULL pointer");
    const unsigned nblk = grid_1d(M, 4, RED_PARTS);
#define LNB_LAUNCH(NCH_)                                                                                               \
    if (x_f32)                                                                                                         \
        hipLaunchKernelGGL((k_layernorm_bwd<NCH_, true>), dim3(nblk), dim3(256), 0, ctx->stream, x, (const u16*)dy, gamma, \
                           dx, part, M, C, eps);                                                                       \
    else                                                                                                               \
        hipLaunchKernelGGL((k_layernorm_bwd<NCH_, false>), dim3(nblk), dim3(256), 0, ctx->stream, x, (const u16*)dy, gamma, \
                           dx, part, M, C, eps)
    if (C <= 512) { LNB_LAUNCH(1); }
    else if (C <= 1024) { LNB_LAUNCH(2); }
    else { LNB_LAUNCH(4); }
#undef LNB_LAUNCH
    CR_LAUNCH_CHECK();
    if (dgamma || dbeta) {
        hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)cr_cdiv(2 * C, 256)), dim3(256), 0, ctx->stream, (const float*)part,
                           (int)nblk, 2 * C, C, dgamma, dbeta, accumulate);
        CR_LAUNCH_CHECK();
    }
    return CR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The training route keeps the residual stream in float32 (the inference path rounds it to bf16 twice per block): LayerNorm
// of a float32 row (vit.hip's k_layernorm with float loads; bf16 out, what the GEMMs read) and x + gamma * y with float32
// x and result, bf16 branch y.
// ---------------------------------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void k_layernorm_f32in(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, u16* __restrict__ y, int64_t M, int C,
                                                         float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * C;
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int i = lane * 8 + 512 * k;
        if (i < C) {
            load_row8<true>(xr, i, v[k]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s += v[k][2 * e] + v[k][2 * e + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (lane * 8 + 512 * k < C) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = v[k][e] - mean;
                q += a * a;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
    const float inv = rsqrtf(q / (float)C + eps);
    u16* yr = y + row * C;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int i = lane * 8 + 512 * k;
        if (i < C) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[k][e] - mean) * inv * gamma[i + e] + beta[i + e];
            *reinterpret_cast<uint4*>(yr + i) = pack8(o);
        }
    }
}

extern "C" int cr_layernorm_f32in(cr_ctx* ctx, const float* x, const float* gamma, const float* beta, void* y, int64_t M, int C,
                                  float eps) {
    CR_CHECK_ARG(ctx && M >= 0 && C > 0 && C % 8 == 0, "cr_layernorm_f32in: bad dims M=%lld C=%d", (long long)M, C);
    CR_CHECK_ARG(C <= 2048, "cr_layernorm_f32in: C=%d > 2048 is not built", C);
    if (M == 0) return CR_OK;
    CR_CHECK_ARG(x && gamma && beta && y, "cr_layernorm_f32in: NULL pointer");
    const dim3 grid((unsigned)cr_cdiv(M, 4));
    if (C <= 512)
        hipLaunchKernelGGL(k_layernorm_f32in<1>, grid, dim3(256), 0, ctx->stream, x, gamma, beta, (u16*)y, M, C, eps);
    else if (C <= 1024)
        hipLaunchKernelGGL(k_layernorm_f32in<2>, grid, dim3(256), 0, ctx->stream, x, gamma, beta, (u16*)y, M, C, eps);
    else
        hipLaunchKernelGGL(k_layernorm_f32in<4>, grid, dim3(256), 0, ctx->stream, x, gamma, beta, (u16*)y, M, C, eps);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

__global__ __launch_bounds__(256) void k_scale_residual_f32(const float* __restrict__ x, const u16* __restrict__ y,
                                                            const float* __restrict__ gamma, float* __restrict__ out, int64_t M,
                                                            int C) {
    const int cg = C >> 3;
    const int64_t total = M * cg;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cg) << 3;
        float a[8], b[8];
        load_row8<true>(x + i * 8, 0, a);
        unpack8(*reinterpret_cast<const uint4*>(y + i * 8), b);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += (gamma ? gamma[c0 + e] : 1.f) * b[e];
        *reinterpret_cast<float4*>(out + i * 8) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4*>(out + i * 8 + 4) = make_float4(a[4], a[5], a[6], a[7]);
    }
}

extern "C" int cr_scale_residual_f32(cr_ctx* ctx, const float* x, const void* y, const float* gamma, float* out, int64_t M, int C) {
    CR_CHECK_ARG(ctx && M >= 0 && C > 0 && C % 8 == 0, "cr_scale_residual_f32: bad dims");
    if (M == 0) return CR_OK;
    CR_CHECK_ARG(x && y && out, "cr_scale_residual_f32: NULL pointer");
    const int64_t total = M * (C >> 3);
    hipLaunchKernelGGL(k_scale_residual_f32, dim3(grid_1d(total, 256, 8192)), dim3(256), 0, ctx->stream, x, (const u16*)y, gamma,
                       out, M, C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// GELU (exact erf form, the expression of vit.hip's k_gelu) out of place -- the training forward keeps the
// pre-activation -- and its backward dx = dy * (Phi(x) + x phi(x)).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gelu_fwd(const u16* __restrict__ x, u16* __restrict__ y, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 v = *reinterpret_cast<const uint4*>(x + i * 8);
        unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = wbf2f((u16)(w[e] & 0xffff)), b = wbf2f((u16)(w[e] >> 16));
            const float ga = 0.5f * a * (1.f + erff(a * 0.70710678118654752f));
            const float gb = 0.5f * b * (1.f + erff(b * 0.70710678118654752f));
            w[e] = (unsigned)wf2bf(ga) | ((unsigned)wf2bf(gb) << 16);
        }
        *reinterpret_cast<uint4*>(y + i * 8) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ __launch_bounds__(256) void k_gelu_bwd(const u16* __restrict__ x, const u16* __restrict__ dy, u16* __restrict__ dx,
                                                  int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        float a[8], d[8], o[8];
        unpack8(*reinterpret_cast<const uint4*>(x + i * 8), a);
        unpack8(*reinterpret_cast<const uint4*>(dy + i * 8), d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float cdf = 0.5f * (1.f + erff(a[e] * 0.70710678118654752f));
            const float pdf = 0.3989422804014327f * __expf(-0.5f * a[e] * a[e]);
            o[e] = d[e] * (cdf + a[e] * pdf);
        }
        *reinterpret_cast<uint4*>(dx + i * 8) = pack8(o);
    }
}

extern "C" int cr_gelu_fwd(cr_ctx* ctx, const void* x, void* y, int64_t n) {
    CR_CHECK_ARG(ctx && n >= 0 && n % 8 == 0, "cr_gelu_fwd: n must be a multiple of 8");
    if (n == 0) return CR_OK;
    CR_CHECK_ARG(x && y, "cr_gelu_fwd: NULL pointer");
    hipLaunchKernelGGL(k_gelu_fwd, dim3(grid_1d(n / 8, 256, 8192)), dim3(256), 0, ctx->stream, (const u16*)x, (u16*)y, n / 8);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_gelu_bwd(cr_ctx* ctx, const void* x, const void* dy, void* dx, int64_t n) {
    CR_CHECK_ARG(ctx && n >= 0 && n % 8 == 0, "cr_gelu_bwd: n must be a multiple of 8");
    if (n == 0) return CR_OK;
    CR_CHECK_ARG(x && dy && dx, "cr_gelu_bwd: NULL pointer");
    hipLaunchKernelGGL(k_gelu_bwd, dim3(grid_1d(n / 8, 256, 8192)), dim3(256), 0, ctx->stream, (const u16*)x, (const u16*)dy,
                       (u16*)dx, n / 8);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerScale + residual backward: out = x + gamma * y, upstream gradient g.  dx = g (no kernel), dy = gamma * g (bf16),
// dgamma = sum_rows g * y: grid.y row chunks write `part` (chunks, C), k_colsum_parts finishes.  gamma NULL: dy only (= g).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_layerscale_bwd(const u16* __restrict__ g, const u16* __restrict__ y,
                                                        const float* __restrict__ gamma, u16* __restrict__ dy,
                                                        float* __restrict__ part, int64_t M, int C, int64_t rows_per) {
    const int j = (blockIdx.x * 128 + threadIdx.x) * 2;
    if (j >= C) return;
    const float g0 = gamma[j], g1 = gamma[j + 1];
    const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = r0 + rows_per < M ? r0 + rows_per : M;
    float a0 = 0.f, a1 = 0.f;
    for (int64_t r = r0; r < r1; ++r) {
        const unsigned gv = *reinterpret_cast<const unsigned*>(g + r * C + j);
        const unsigned yv = *reinterpret_cast<const unsigned*>(y + r * C + j);
        const float ga = wbf2f((u16)(gv & 0xffff)), gb = wbf2f((u16)(gv >> 16));
        a0 += ga * wbf2f((u16)(yv & 0xffff));
        a1 += gb * wbf2f((u16)(yv >> 16));
        *reinterpret_cast<unsigned*>(dy + r * C + j) = (unsigned)wf2bf(g0 * ga) | ((unsigned)wf2bf(g1 * gb) << 16);
    }
    part[(size_t)blockIdx.y * C + j] = a0;
    part[(size_t)blockIdx.y * C + j + 1] = a1;
}

extern "C" int cr_layerscale_bwd(cr_ctx* ctx, const void* g, const void* y, const float* gamma, void* dy, float* dgamma,
                                 float* part, int64_t M, int C, int accumulate) {
    CR_CHECK_ARG(ctx && M >= 0 && C > 0 && C % 8 == 0, "cr_layerscale_bwd: bad dims");
    if (M == 0) return CR_OK;
    CR_CHECK_ARG(g && y && gamma && dy && dgamma && part, "cr_layerscale_bwd: NULL pointer");
    const int64_t rows_per = cr_cdiv(M, RED_PARTS) < 8 ? 8 : cr_cdiv(M, RED_PARTS);
    const int chunks = (int)cr_cdiv(M, rows_per);
    hipLaunchKernelGGL(k_layerscale_bwd, dim3((unsigned)cr_cdiv(C, 256), (unsigned)chunks), dim3(128), 0, ctx->stream,
                       (const u16*)g, (const u16*)y, gamma, (u16*)dy, part, M, C, rows_per);
    CR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)cr_cdiv(C, 256)), dim3(256), 0, ctx->stream, (const float*)part, chunks, C, C,
                       dgamma, (float*)nullptr, accumulate);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward of k_resize_bilinear_ac (vit.hip) as a gather: one thread per input pixel and 8 channels sums the output pixels
// that read it.  The candidates come from inverting the source coordinate with a margin; each candidate's (y0, y1, ly) is
// then recomputed exactly, so a pixel is never counted for a neighbour it did not read.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void resize_range(int i, float s, int no, int* lo, int* hi) {
    if (s > 0.f) {
        const int a = (int)floorf((float)(i - 1) / s) - 1, b = (int)ceilf((float)(i + 1) / s) + 1;
        *lo = a < 0 ? 0 : a;
        *hi = b > no - 1 ? no - 1 : b;
    } else {
        *lo = 0;
        *hi = no - 1;
    }
}
// weight of input index i in output index o: the source coordinate o (n-1)/(no-1) as an exact rational (integer quotient
// and remainder), so the weight carries one float32 rounding instead of the 2^-24 * coordinate of a float product
__device__ __forceinline__ float resize_weight(int o, int no, int n, int i) {
    int p0 = 0;
    float l = 0.f;
    if (no > 1) {
        const int64_t num = (int64_t)o * (n - 1), den = no - 1;
        p0 = (int)(num / den);
        l = (float)(num - (int64_t)p0 * den) / (float)den;
    }
    const int p1 = min(p0 + 1, n - 1);
    return (p0 == i ? 1.f - l : 0.f) + (p1 == i ? l : 0.f);
}

__global__ __launch_bounds__(256) void k_resize_bilinear_ac_bwd(const u16* __restrict__ dy, u16* __restrict__ dx, int B, int h,
                                                                int w, int Ho, int Wo, int C) {
    const int cg = C >> 3;
    const int64_t total = (int64_t)B * h * w * cg;
    const float sy = Ho > 1 ? (float)(h - 1) / (float)(Ho - 1) : 0.f;
    const float sx = Wo > 1 ? (float)(w - 1) / (float)(Wo - 1) : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cg) << 3;
        int64_t r = i / cg;
        const int ix = (int)(r % w); r /= w;
        const int iy = (int)(r % h);
        const int b = (int)(r / h);
        int ylo, yhi, xlo, xhi;
        resize_range(iy, sy, Ho, &ylo, &yhi);
        resize_range(ix, sx, Wo, &xlo, &xhi);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const u16* p = dy + (size_t)b * Ho * Wo * C + c0;
        for (int oy = ylo; oy <= yhi; ++oy) {
            const float wy = resize_weight(oy, Ho, h, iy);
            if (wy == 0.f) continue;
            for (int ox = xlo; ox <= xhi; ++ox) {
                const float wx = resize_weight(ox, Wo, w, ix);
                if (wx == 0.f) continue;
                float d[8];
                unpack8(*reinterpret_cast<const uint4*>(p + ((size_t)oy * Wo + ox) * C), d);
                const float ww = wy * wx;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += ww * d[e];
            }
        }
        *reinterpret_cast<uint4*>(dx + i * 8) = pack8(acc);
    }
}

extern "C" int cr_resize_bilinear_ac_bwd(cr_ctx* ctx, const void* dy, void* dx, int B, int h, int w, int Ho, int Wo, int C) {
    CR_CHECK_ARG(ctx && B >= 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 8 == 0, "cr_resize_bilinear_ac_bwd: bad dims");
    if (B == 0) return CR_OK;
    CR_CHECK_ARG(dy && dx, "cr_resize_bilinear_ac_bwd: NULL pointer");
    const int64_t total = (int64_t)B * h * w * (C >> 3);
    hipLaunchKernelGGL(k_resize_bilinear_ac_bwd, dim3(grid_1d(total, 256, 16384)), dim3(256), 0, ctx->stream, (const u16*)dy,
                       (u16*)dx, B, h, w, Ho, Wo, C);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Masked depth reduction over (pred, target, valid), (B, HW) each: per image the ten sums behind SiLogLoss (util/loss.py)
// and eval_depth (util/metric.py), with d = p - t and dl = log p - log t over the valid pixels:
//   0 count, 1 sum dl, 2 sum dl^2, 3 sum |d|/t, 4 sum d^2/t, 5 sum d^2, 6 sum |log10 p - log10 t|,
//   7..9 count of max(t/p, p/t) < 1.25^k, k = 1, 2, 3 (float32 comparisons like the reference's).
// One workgroup per image; per-thread float64 partial sums in a strided walk, then a fixed tree through LDS.
// ---------------------------------------------------------------------------------------------------------------------
#define DR_N 10
#define DR_T 512

__global__ __launch_bounds__(DR_T) void k_depth_reduce(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const unsigned char* __restrict__ valid, double* __restrict__ sums,
                                                       int64_t HW) {
    __shared__ double sh[DR_T];
    const float* p = pred + (size_t)blockIdx.x * HW;
    const float* t = target + (size_t)blockIdx.x * HW;
    const unsigned char* m = valid + (size_t)blockIdx.x * HW;
    double a[DR_N];
#pragma unroll
    for (int k = 0; k < DR_N; ++k) a[k] = 0.0;
    const float th1 = 1.25f, th2 = 1.25f * 1.25f, th3 = 1.25f * 1.25f * 1.25f;
    for (int64_t i = threadIdx.x; i < HW; i += DR_T) {
        if (!m[i]) continue;
        const float pv = p[i], tv = t[i];
        const float d = pv - tv, dl = logf(pv) - logf(tv);
        const float th = fmaxf(tv / pv, pv / tv);
        a[0] += 1.0;
        a[1] += (double)dl;
        a[2] += (double)dl * (double)dl;
        a[3] += (double)(fabsf(d) / tv);
        a[4] += (double)(d * d / tv);
        a[5] += (double)d * (double)d;
        a[6] += (double)fabsf(log10f(pv) - log10f(tv));
        a[7] += th < th1 ? 1.0 : 0.0;
        a[8] += th < th2 ? 1.0 : 0.0;
        a[9] += th < th3 ? 1.0 : 0.0;
    }
    for (int k = 0; k < DR_N; ++k) {
        sh[threadIdx.x] = a[k];
        __syncthreads();
        for (int off = DR_T / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[(size_t)blockIdx.x * DR_N + k] = sh[0];
        __syncthreads();
    }
}

extern "C" int cr_depth_reduce(cr_ctx* ctx, const float* pred, const float* target, const unsigned char* valid, double* sums, int B,
                               int64_t HW) {
    CR_CHECK_ARG(ctx && B >= 0 && HW >= 0, "cr_depth_reduce: bad dims");
    if (B == 0) return CR_OK;
    CR_CHECK_ARG(sums && (HW == 0 || (pred && target && valid)), "cr_depth_reduce: NULL pointer");
    hipLaunchKernelGGL(k_depth_reduce, dim3((unsigned)B), dim3(DR_T), 0, ctx->stream, pred, target, valid, sums, HW);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

// d SiLog / d pred: with n valid pixels, S1 = sum dl and L the loss, dL/dp_i = (dl_i / n - lambda S1 / n^2) / (L p_i) on valid
// pixels and exactly 0 elsewhere.  coef (device, f32): {gout / (n L), gout * lambda * S1 / (n^2 L)}.
__global__ __launch_bounds__(256) void k_silog_bwd(const float* __restrict__ pred, const float* __restrict__ target,
                                                   const unsigned char* __restrict__ valid, const float* __restrict__ coef,
                                                   float* __restrict__ dpred, int64_t n) {
    const float ca = coef[0], cb = coef[1];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float o = 0.f;
        if (valid[i]) {
            const float pv = pred[i];
            o = (ca * (logf(pv) - logf(target[i])) - cb) / pv;
        }
        dpred[i] = o;
    }
}

extern "C" int cr_silog_bwd(cr_ctx* ctx, const float* pred, const float* target, const unsigned char* valid, const float* coef,
                            float* dpred, int64_t n) {
    CR_CHECK_ARG(ctx && n >= 0, "cr_silog_bwd: bad dims");
    if (n == 0) return CR_OK;
    CR_CHECK_ARG(pred && target && valid && coef && dpred, "cr_silog_bwd: NULL pointer");
    hipLaunchKernelGGL(k_silog_bwd, dim3(grid_1d(n, 256, 8192)), dim3(256), 0, ctx->stream, pred, target, valid, coef, dpred, n);
    CR_LAUNCH_CHECK();
    return CR_OK;
}
