// The six ablation proposal samplers of the proposal method (ProposalNetwork/proposals/proposals.py:20-336 of the
// reference, chosen by name in cubercnn/modeling/roi_heads/roi_heads.py:283-302) for the objects of a whole batch in
// one launch: one workgroup per object like k_propose (geometry.hip), img_idx selects the object's depth map and K.
// gfx950 only; wave = 64.
//
// Every random variate is an input (as in cr_propose): the kernels hold arithmetic only, so recorded draws replay
// through them.  This translation unit is compiled with -ffp-contract=off: the float32 operation order is that of the
// host restatement in ProposalNetwork/proposals/proposals.py (which tests/test_proposal_variants.py pins to the
// reference's recorded draws).
//
//   random    proposals.py:20-45     everything uniform
//   xy        proposals.py:47-91     x / y on a line through the inner half of the box (normalised image space)
//   z         proposals.py:93-135    as xy, z on a line between the 10 % and 90 % quantiles of the box's depth patch
//   dim       proposals.py:137-197   centre from the depth rays like `propose`, uniform dimensions
//   aspect    proposals.py:199-270   as dim, height and length = width x one of seven ratios per object
//   rotation  proposals.py:272-336   as `propose` (truncated-normal dimensions) with a random basis (= :398-400)
//   basis     ProposalNetwork/utils/utils.py:62-69
//   rays, median / std, truncated normals: the arithmetic of k_propose (proposals.py:338-424, utils.py:42-60,170-177)
#include "cr_common.h"
#include <math.h>

#define PS_T 256                 // threads per workgroup (4 waves)
#define PS_W (PS_T / 64)
#define PS_MAXP 1024
#define PS_SLOTS (PS_MAXP / PS_T)

struct SamplerArgs {
    const float* boxes;          // (N,4)
    const int32_t* img_idx;      // (N)
    const float* depth;          // (B,H,W)
    const float* prior_mu;       // (N,3)
    const float* prior_sigma;    // (N,3)
    const float* K;              // (B,3,3)
    const float* uniforms;       // (U,N,P)
    const float* ctr_normals;    // (3,N,P)
    const float* dim_normals;    // (rounds,3,N,P)
    const int32_t* ratio_idx;    // (N,2)
    const float* basis;          // (N,P,3,3)
    float* out_cubes;            // (N,P,15)
    int32_t* out_exhausted;      // (1)
    int B, H, W, N, P, rounds;
    float half_w, scale_w, half_h, scale_h;      // pixel_to_normalised_space: (v - half) * scale
};

__device__ __forceinline__ float ps_nan() { return __builtin_nanf(""); }

__device__ __forceinline__ double ps_block_sum_f64(double val, double* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) val += __shfl_down(val, off, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) scratch[w] = val;
    __syncthreads();
    double r = scratch[0];
#pragma unroll
    for (int i = 1; i < PS_W; ++i) r += scratch[i];
    return r;
}

// in-LDS bitonic sort of 1024 floats (ascending; padded with +inf)
__device__ __forceinline__ void ps_bitonic_sort_1024(float* a) {
    for (int k = 2; k <= PS_MAXP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < PS_MAXP / 2; t += PS_T) {
                const int i = ((t / j) * 2 * j) + (t % j);
                const int l = i + j;
                const bool up = ((i & k) == 0);
                const float x = a[i], y = a[l];
                if ((x > y) == up) { a[i] = y; a[l] = x; }
            }
        }
    }
    __syncthreads();
}

// rescale_interval(u, 0.05, 2), proposals.py:12-14: (min - max) * u + max
__device__ __forceinline__ float ps_uniform_dim(float u) { return (float)(0.05 - 2.0) * u + 2.0f; }

// ---- depth rays -> lower median and unbiased std of x, y, z over the P samples -> centres (k_propose's arithmetic) ----
// vx / vy / vz hold the ray samples of this thread's slots (z already + l/2); on return they hold the centres.
__device__ __forceinline__ void ps_ray_centres(const SamplerArgs& a, const int obj, float* vx, float* vy, float* vz) {
    __shared__ float s_sort[PS_MAXP];
    __shared__ double s_red64[PS_W];
    __shared__ float s_stat[6];       // median x,y,z ; std x,y,z
    const int tid = threadIdx.x, P = a.P;
    for (int k = 0; k < 3; ++k) {
        __syncthreads();
        double lsum = 0.0;
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            const float v = k == 0 ? vx[s] : (k == 1 ? vy[s] : vz[s]);
            s_sort[p] = p < P ? v : INFINITY;
            if (p < P) lsum += (double)v;
        }
        const double mean = ps_block_sum_f64(lsum, s_red64) / (double)P;
        double lsq = 0.0;
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            if (p < P) {
                const double dv = (double)(k == 0 ? vx[s] : (k == 1 ? vy[s] : vz[s])) - mean;
                lsq += dv * dv;
            }
        }
        const double var = ps_block_sum_f64(lsq, s_red64) / (double)(P - 1);
        ps_bitonic_sort_1024(s_sort);
        if (tid == 0) {
            s_stat[k] = s_sort[(P - 1) / 2];
            s_stat[3 + k] = (float)sqrt(var);
        }
    }
    __syncthreads();
    const float mx = 1.15f * s_stat[0] + 0.0f, sx = s_stat[3] * 1.2f;
    const float my = 1.1f * s_stat[1] + 0.0f, sy = s_stat[4] * 0.8f;
    const float mz = 0.85f * s_stat[2] + 0.35f, sz = s_stat[5] * 1.2f;
#pragma unroll
    for (int s = 0; s < PS_SLOTS; ++s) {
        const int p = s * PS_T + tid;
        if (p < P) {
            vx[s] = mx + sx * a.ctr_normals[((size_t)0 * a.N + obj) * P + p];
            vy[s] = my + sy * a.ctr_normals[((size_t)1 * a.N + obj) * P + p];
            vz[s] = mz + sz * a.ctr_normals[((size_t)2 * a.N + obj) * P + p];
        }
    }
}

// ---- torch.quantile(patch, [0.1, 0.9], interpolation='linear') in float32 ------------------------------------------
// Selection, not sorting (the patch can be the whole image): a 4-pass 8-bit radix select over the order-preserving
// integer image of the float bits, in the manner of k_box_median (weak.hip), for the lower order statistic of both
// quantiles in the same passes; a fifth pass counts the elements <= each of them and finds the smallest element above,
// which gives the upper order statistic, and looks for NaNs.
__device__ __forceinline__ unsigned ps_f2ord(float f) {      // monotone float -> uint
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ps_ord2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// a Python slice bound on an axis of length L
__device__ __forceinline__ int ps_slice_bound(int v, int L) {
    if (v < 0) v += L;
    return min(max(v, 0), L);
}

// lerp of ATen (weight < 0.5 ? a + w (b - a) : b - (b - a)(1 - w)), fused like its vectorised CPU kernel
__device__ __forceinline__ float ps_lerp(float lo, float hi, float w) {
    return w < 0.5f ? fmaf(w, hi - lo, lo) : fmaf(w - 1.0f, hi - lo, hi);
}

// q[0], q[1] = the 10 % and 90 % quantiles of depth[y1:y2, x1:x2] (one image's map, bounds already those of the slice);
// NaN for an empty patch or one that holds a NaN.  All threads of the workgroup call it; the result is in LDS.
__device__ __forceinline__ void ps_patch_quantiles(const float* __restrict__ depth, const int W, const int x1, const int y1,
                                                   const int bw, const int bh, float* s_q) {
    __shared__ unsigned s_hist[2][256];
    __shared__ unsigned s_prefix[2], s_k[2], s_le[2], s_next[2], s_nan;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long n = (long)bw * bh;
    if (n == 0) {                                  // uniform over the workgroup
        if (tid == 0) s_q[0] = s_q[1] = ps_nan();
        __syncthreads();
        return;
    }
    // ranks q (n - 1) in float32 like ATen's quantile_compute; below = trunc, above = ceil, weight = rank - below
    const float rk0 = 0.1f * (float)(n - 1), rk1 = 0.9f * (float)(n - 1);
    const long lo0 = (long)rk0, lo1 = (long)rk1;
    const float* base = depth + (size_t)y1 * W + x1;
    if (tid == 0) {
        s_prefix[0] = s_prefix[1] = 0u;
        s_k[0] = (unsigned)lo0; s_k[1] = (unsigned)lo1;
        s_le[0] = s_le[1] = 0u;
        s_next[0] = s_next[1] = 0xffffffffu;
        s_nan = 0u;
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        s_hist[0][tid] = 0u;                       // PS_T == 256 bins
        s_hist[1][tid] = 0u;
        __syncthreads();
        const unsigned pre0 = s_prefix[0], pre1 = s_prefix[1];
        const unsigned hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        // run-length accumulation (see k_box_median): neighbouring depths share their high bytes
        int cur0 = -1, cur1 = -1;
        unsigned run0 = 0, run1 = 0;
        for (int r = wave; r < bh; r += PS_W) {
            const float* row = base + (size_t)r * W;
            for (int c = lane; c < bw; c += 64) {
                const unsigned key = ps_f2ord(row[c]);
                const int bin = (int)((key >> shift) & 255u);
                const int bin0 = (key & hi_mask) == pre0 ? bin : -1;
                const int bin1 = (key & hi_mask) == pre1 ? bin : -1;
                if (bin0 == cur0) ++run0;
                else { if (cur0 >= 0) atomicAdd(&s_hist[0][cur0], run0); cur0 = bin0; run0 = 1; }
                if (bin1 == cur1) ++run1;
                else { if (cur1 >= 0) atomicAdd(&s_hist[1][cur1], run1); cur1 = bin1; run1 = 1; }
            }
        }
        if (cur0 >= 0) atomicAdd(&s_hist[0][cur0], run0);
        if (cur1 >= 0) atomicAdd(&s_hist[1][cur1], run1);
        __syncthreads();
        if (wave < 2) {
            // wave t scans the 256 bins of target t: each lane owns 4 consecutive bins
            const unsigned* h = s_hist[wave];
            const unsigned h0 = h[4 * lane], h1 = h[4 * lane + 1], h2 = h[4 * lane + 2], h3 = h[4 * lane + 3];
            const unsigned mine = h0 + h1 + h2 + h3;
            unsigned incl = mine;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(incl, off, 64);
                if (lane >= off) incl += v;
            }
            const unsigned excl = incl - mine, k = s_k[wave];
            if (k >= excl && k < incl) {                   // exactly one lane
                unsigned run = excl, bin;
                if (k < run + h0) bin = 0;
                else if (k < (run += h0) + h1) bin = 1;
                else if (k < (run += h1) + h2) bin = 2;
                else { run += h2; bin = 3; }
                s_prefix[wave] = (wave == 0 ? pre0 : pre1) | ((4u * lane + bin) << shift);
                s_k[wave] = k - run;
            }
        }
        __syncthreads();
    }
    const unsigned key0 = s_prefix[0], key1 = s_prefix[1];
    unsigned le0 = 0, le1 = 0, nx0 = 0xffffffffu, nx1 = 0xffffffffu, anynan = 0;
    for (int r = wave; r < bh; r += PS_W) {
        const float* row = base + (size_t)r * W;
        for (int c = lane; c < bw; c += 64) {
            const float v = row[c];
            const unsigned key = ps_f2ord(v);
            anynan |= (v != v) ? 1u : 0u;
            if (key <= key0) ++le0; else nx0 = min(nx0, key);
            if (key <= key1) ++le1; else nx1 = min(nx1, key);
        }
    }
    if (le0) atomicAdd(&s_le[0], le0);
    if (le1) atomicAdd(&s_le[1], le1);
    if (nx0 != 0xffffffffu) atomicMin(&s_next[0], nx0);
    if (nx1 != 0xffffffffu) atomicMin(&s_next[1], nx1);
    if (anynan) atomicOr(&s_nan, 1u);
    __syncthreads();
    if (tid < 2) {
        const float rk = tid == 0 ? rk0 : rk1;
        const long lo = tid == 0 ? lo0 : lo1;
        const long hi = (long)ceilf(rk);
        const unsigned key = tid == 0 ? key0 : key1;
        const float below = ps_ord2f(key);
        // sorted[lo + 1] is the same value when at least lo + 2 elements are <= it, else the smallest element above
        const float above = (hi == lo || (long)s_le[tid] >= lo + 2) ? below : ps_ord2f(s_next[tid]);
        s_q[tid] = s_nan ? ps_nan() : ps_lerp(below, above, rk - (float)lo);
    }
    __syncthreads();
}

enum { M_RANDOM = CR_SAMPLER_RANDOM, M_XY = CR_SAMPLER_XY, M_Z = CR_SAMPLER_Z, M_DIM = CR_SAMPLER_DIM,
       M_ASPECT = CR_SAMPLER_ASPECT, M_ROTATION = CR_SAMPLER_ROTATION };

template <int MODE>
__global__ __launch_bounds__(PS_T) void k_propose_sampler(const SamplerArgs a) {
    constexpr bool RAYS = MODE == M_DIM || MODE == M_ASPECT || MODE == M_ROTATION;
    __shared__ float s_q[2];
    const int obj = blockIdx.x, tid = threadIdx.x, P = a.P, N = a.N, H = a.H, W = a.W;
    const size_t NP = (size_t)N * P;
    const size_t row = (size_t)obj * P;            // offset of the object inside one (N,P) plane of variates
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (MODE != M_RANDOM) { b0 = a.boxes[obj * 4 + 0]; b1 = a.boxes[obj * 4 + 1]; b2 = a.boxes[obj * 4 + 2]; b3 = a.boxes[obj * 4 + 3]; }
    const float* depth = a.depth;
    const float* Kmat = a.K;
    if (MODE == M_Z || RAYS) {
        const int im = min(max(a.img_idx[obj], 0), a.B - 1);
        depth += (size_t)im * H * W;
        if (RAYS) Kmat += im * 9;
    }

    const float wd = b2 - b0, ht = b3 - b1;
    const float x_lo = b0 + wd / 4.0f, x_hi = b2 - wd / 4.0f;
    const float y_lo = b1 + ht / 4.0f, y_hi = b3 - ht / 4.0f;

    float vx[PS_SLOTS], vy[PS_SLOTS], vz[PS_SLOTS], dims[PS_SLOTS][3];

    // ---- dimensions ----
    if constexpr (MODE == M_ROTATION) {
        const float mu[3] = {a.prior_mu[obj * 3], a.prior_mu[obj * 3 + 1], a.prior_mu[obj * 3 + 2]};
        const float sg[3] = {a.prior_sigma[obj * 3], a.prior_sigma[obj * 3 + 1] * 1.1f, a.prior_sigma[obj * 3 + 2]};
        const float hi[3] = {mu[0] + 2.0f * a.prior_sigma[obj * 3], mu[1] + 2.2f * a.prior_sigma[obj * 3 + 1],
                             mu[2] + 2.0f * a.prior_sigma[obj * 3 + 2]};
        int exhausted = 0;
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            if (p < P) {
                // truncated normals for w,h,l with `rounds` pre-drawn rejection rounds (utils.py:42-60)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float v = mu[k] + sg[k] * a.dim_normals[(size_t)k * NP + row + p];
                    for (int r = 1; r < a.rounds && (v < 0.05f || v > hi[k]); ++r)
                        v = mu[k] + sg[k] * a.dim_normals[((size_t)r * 3 + k) * NP + row + p];
                    if (v < 0.05f || v > hi[k]) exhausted++;
                    dims[s][k] = v;
                }
            }
        }
        if (exhausted) atomicAdd(a.out_exhausted, exhausted);
    } else if constexpr (MODE == M_ASPECT) {
        const float ratios[7] = {(float)0.33, (float)0.66, 1.0f, (float)1.33, (float)1.67, 2.0f, 3.0f};
        const float r1 = ratios[min(max(a.ratio_idx[obj * 2 + 0], 0), 6)];
        const float r2 = ratios[min(max(a.ratio_idx[obj * 2 + 1], 0), 6)];
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            if (p < P) {
                const float w = ps_uniform_dim(a.uniforms[row + p]);
                dims[s][0] = w; dims[s][1] = w * r1; dims[s][2] = w * r2;
            }
        }
    } else {
        constexpr int U0 = MODE == M_RANDOM ? 3 : (MODE == M_XY ? 1 : 0);      // the first of the three dimension uniforms
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            if (p < P) {
#pragma unroll
                for (int k = 0; k < 3; ++k) dims[s][k] = ps_uniform_dim(a.uniforms[(size_t)(U0 + k) * NP + row + p]);
            }
        }
    }

    // ---- centres ----
    if constexpr (MODE == M_RANDOM) {
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            if (p < P) {
                vx[s] = a.uniforms[(size_t)0 * NP + row + p] * 4.0f - 2.0f;
                vy[s] = a.uniforms[(size_t)1 * NP + row + p] * 2.0f - 1.0f;
                vz[s] = a.uniforms[(size_t)2 * NP + row + p] * 4.0f + 1.0f;
            }
        }
    } else if constexpr (MODE == M_XY || MODE == M_Z) {
        // pixel_to_normalised_space (conversions.py:50-67) of the inner half's ends, then vectorized_linspace
        const float xt0 = (x_lo - a.half_w) * a.scale_w, xt1 = (x_hi - a.half_w) * a.scale_w;
        const float yt0 = (y_lo - a.half_h) * a.scale_h, yt1 = (y_hi - a.half_h) * a.scale_h;
        const float x_sp = (xt1 - xt0) / (float)(P - 1), y_sp = (yt1 - yt0) / (float)(P - 1);
        float z0 = 0.f, z1 = 0.f, z_sp = 0.f;
        if constexpr (MODE == M_Z) {
            // depth[int(y1):int(y2), int(x1):int(x2)] with Python's slice rules
            const int sx1 = ps_slice_bound((int)truncf(b0), W), sx2 = ps_slice_bound((int)truncf(b2), W);
            const int sy1 = ps_slice_bound((int)truncf(b1), H), sy2 = ps_slice_bound((int)truncf(b3), H);
            ps_patch_quantiles(depth, W, sx1, sy1, max(sx2 - sx1, 0), max(sy2 - sy1, 0), s_q);
            z0 = s_q[0]; z1 = s_q[1];
            z_sp = (z1 - z0) / (float)(P - 1);
        }
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            if (p < P) {
                vx[s] = (float)p * x_sp + xt0;
                vy[s] = (float)p * y_sp + yt0;
                if (MODE == M_XY) vz[s] = a.uniforms[row + p] * 4.0f + 1.0f;
                // torch.linspace: symmetric fill (first half from the start, second half from the end)
                else vz[s] = p < P / 2 ? z0 + z_sp * (float)p : z1 - z_sp * (float)(P - p - 1);
            }
        }
    } else {
        const float K00 = Kmat[0], K02 = Kmat[2], K12 = Kmat[5];
        const float x_sp = (x_hi - x_lo) / (float)(P - 1), y_sp = (y_hi - y_lo) / (float)(P - 1);
#pragma unroll
        for (int s = 0; s < PS_SLOTS; ++s) {
            const int p = s * PS_T + tid;
            vx[s] = vy[s] = vz[s] = INFINITY;
            if (p < P) {
                // vectorized_linspace(...).long(): trunc toward zero (utils.py:170-177, proposals.py:360-363)
                const long xg = (long)truncf((float)p * x_sp + x_lo);
                const long yg = (long)truncf((float)p * y_sp + y_lo);
                long xi = xg < 0 ? xg + W : xg, yi = yg < 0 ? yg + H : yg;      // python negative-index wrap
                xi = min(max(xi, 0L), (long)W - 1);
                yi = min(max(yi, 0L), (long)H - 1);
                const float d = depth[yi * W + xi];
                const float ox = (float)xg - K02, oy = (float)yg - K12, adj = K00;
                const float ang_x = atan2f(ox, adj);
                const float dxc = sqrtf(ox * ox + adj * adj);
                const float ang_d = atan2f(oy, dxc);
                const float y = d * sinf(ang_d);
                const float dx = sqrtf(d * d - y * y);
                const float x = dx * sinf(ang_x);
                const float zt = sqrtf(dx * dx - x * x);
                vx[s] = x; vy[s] = y; vz[s] = zt + dims[s][2] / 2.0f;
            }
        }
        ps_ray_centres(a, obj, vx, vy, vz);
    }

    // ---- random orthonormal basis (utils.py:62-69) and the store ----
#pragma unroll
    for (int s = 0; s < PS_SLOTS; ++s) {
        const int p = s * PS_T + tid;
        if (p < P) {
            const float* g = a.basis + (row + p) * 9;
            float r[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float g0 = g[3 * i], g1 = g[3 * i + 1], g2 = g[3 * i + 2];
                const float nrm = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
                r[i][0] = g0 / nrm; r[i][1] = g1 / nrm; r[i][2] = g2 / nrm;
            }
            // row0 = normalise(row1 x row2), row1 = normalise(row2 x row0)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float* u = r[(i + 1) % 3];
                const float* v = r[(i + 2) % 3];
                const float c0 = u[1] * v[2] - u[2] * v[1], c1 = u[2] * v[0] - u[0] * v[2], c2 = u[0] * v[1] - u[1] * v[0];
                const float nrm = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
                r[i][0] = c0 / nrm; r[i][1] = c1 / nrm; r[i][2] = c2 / nrm;
            }
            float* o = a.out_cubes + (row + p) * 15;
            o[0] = vx[s]; o[1] = vy[s]; o[2] = vz[s];
            o[3] = dims[s][0]; o[4] = dims[s][1]; o[5] = dims[s][2];
#pragma unroll
            for (int i = 0; i < 3; ++i) { o[6 + 3 * i] = r[i][0]; o[7 + 3 * i] = r[i][1]; o[8 + 3 * i] = r[i][2]; }
        }
    }
}

extern "C" int cr_propose_sampler_batched(cr_ctx* ctx, int mode, const float* boxes, const int32_t* img_idx, int64_t N,
                                          const float* depth, int B, int H, int W, const float* prior_mu,
                                          const float* prior_sigma, const float* K, float im_w, float im_h, int64_t P,
                                          const float* uniforms, const float* ctr_normals, const float* dim_normals,
                                          int rounds, const int32_t* ratio_idx, const float* basis, float* out_cubes,
                                          int32_t* out_exhausted) {
    CR_CHECK_ARG(ctx != nullptr, "cr_propose_sampler_batched: ctx is NULL");
    CR_CHECK_ARG(mode >= CR_SAMPLER_RANDOM && mode <= CR_SAMPLER_ROTATION, "cr_propose_sampler_batched: unknown mode %d", mode);
    CR_CHECK_ARG(N >= 0 && B >= 1, "cr_propose_sampler_batched: bad N / B");
    CR_CHECK_ARG(out_exhausted != nullptr, "cr_propose_sampler_batched: out_exhausted is NULL");
    CR_HIP(hipMemsetAsync(out_exhausted, 0, sizeof(int32_t), ctx->stream));
    if (N == 0) return CR_OK;
    CR_CHECK_ARG(P >= 2 && P <= PS_MAXP, "cr_propose_sampler_batched: P=%lld outside [2,%d]", (long long)P, PS_MAXP);
    CR_CHECK_ARG(N * P < (1ll << 31) / 15, "cr_propose_sampler_batched: N x P too large");
    CR_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "cr_propose_sampler_batched: bad depth shape");
    const bool rays = mode == CR_SAMPLER_DIM || mode == CR_SAMPLER_ASPECT || mode == CR_SAMPLER_ROTATION;
    const bool lines = mode == CR_SAMPLER_XY || mode == CR_SAMPLER_Z;
    CR_CHECK_ARG(basis && out_cubes, "cr_propose_sampler_batched: NULL basis / out_cubes");
    CR_CHECK_ARG(mode == CR_SAMPLER_RANDOM || boxes, "cr_propose_sampler_batched: NULL boxes");
    CR_CHECK_ARG(!(rays || mode == CR_SAMPLER_Z) || (img_idx && depth), "cr_propose_sampler_batched: NULL img_idx / depth");
    CR_CHECK_ARG(!rays || (K && ctr_normals), "cr_propose_sampler_batched: NULL K / ctr_normals");
    CR_CHECK_ARG(!lines || (im_w > 0.0f && im_h > 0.0f), "cr_propose_sampler_batched: bad image shape");
    CR_CHECK_ARG(mode == CR_SAMPLER_ROTATION || uniforms, "cr_propose_sampler_batched: NULL uniforms");
    CR_CHECK_ARG(mode != CR_SAMPLER_ASPECT || ratio_idx, "cr_propose_sampler_batched: NULL ratio_idx");
    if (mode == CR_SAMPLER_ROTATION) {
        CR_CHECK_ARG(rounds >= 1, "cr_propose_sampler_batched: rounds must be >= 1");
        CR_CHECK_ARG(prior_mu && prior_sigma && dim_normals, "cr_propose_sampler_batched: NULL priors / dim_normals");
    }
    SamplerArgs a;
    a.boxes = boxes; a.img_idx = img_idx; a.depth = depth; a.prior_mu = prior_mu; a.prior_sigma = prior_sigma; a.K = K;
    a.uniforms = uniforms; a.ctr_normals = ctr_normals; a.dim_normals = dim_normals; a.ratio_idx = ratio_idx; a.basis = basis;
    a.out_cubes = out_cubes; a.out_exhausted = out_exhausted;
    a.B = B; a.H = H; a.W = W; a.N = (int)N; a.P = (int)P; a.rounds = rounds;
    // conversions.py:50-67 on im_shape = (w, h) with the normalised extents 3 and 2: python floats, then float32 tensor ops
    a.half_w = (float)(0.5 * (double)im_w); a.scale_w = lines ? (float)(3.0 / (double)im_w) : 0.0f;
    a.half_h = (float)(0.5 * (double)im_h); a.scale_h = lines ? (float)(2.0 / (double)im_h) : 0.0f;
    const dim3 grid((unsigned)N), block(PS_T);
    switch (mode) {
        case CR_SAMPLER_RANDOM: hipLaunchKernelGGL(k_propose_sampler<M_RANDOM>, grid, block, 0, ctx->stream, a); break;
        case CR_SAMPLER_XY: hipLaunchKernelGGL(k_propose_sampler<M_XY>, grid, block, 0, ctx->stream, a); break;
        case CR_SAMPLER_Z: hipLaunchKernelGGL(k_propose_sampler<M_Z>, grid, block, 0, ctx->stream, a); break;
        case CR_SAMPLER_DIM: hipLaunchKernelGGL(k_propose_sampler<M_DIM>, grid, block, 0, ctx->stream, a); break;
        case CR_SAMPLER_ASPECT: hipLaunchKernelGGL(k_propose_sampler<M_ASPECT>, grid, block, 0, ctx->stream, a); break;
        default: hipLaunchKernelGGL(k_propose_sampler<M_ROTATION>, grid, block, 0, ctx->stream, a); break;
    }
    CR_LAUNCH_CHECK();
    return CR_OK;
}
