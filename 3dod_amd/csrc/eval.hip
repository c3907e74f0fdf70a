// AP2D / AP3D evaluation of a whole dataset (cubercnn/evaluation/omni3d_evaluation.py of the reference, computeIoU :1360-1432
// and evaluateImg :1434-1553; the protocol is pycocotools' COCOeval [third-party], restated): every IoU in one launch, every
// greedy match in one launch.
// A group is one (image, category) pair with at least one detection or ground-truth box.  Groups are packed CSR-style:
// dt_off / gt_off (n_groups + 1) index the detection / ground-truth arrays, detections already sorted by descending score and
// cut to maxDets[-1]; the IoU matrix of group g is row-major D_g x G_g float64 at iou_off[g].
// Built with -ffp-contract=off: the 2D IoU is bit-equal to the host's iou_xywh (numpy float64, no fused multiply-add).
#include "cr_common.h"
#include "eval_iou3d.h"

// pycocotools maskUtils.iou for [x,y,w,h] boxes (iscrowd = 0) with the operation order of iou_xywh
__device__ __forceinline__ double iou_xywh_pair(const double* __restrict__ d, const double* __restrict__ g) {
    const double x1 = fmax(d[0], g[0]), y1 = fmax(d[1], g[1]);
    const double x2 = fmin(d[0] + d[2], g[0] + g[2]), y2 = fmin(d[1] + d[3], g[1] + g[3]);
    double w = x2 - x1, h = y2 - y1;
    w = w > 0.0 ? w : 0.0;
    h = h > 0.0 ? h : 0.0;
    const double inter = w * h;
    const double uni = (d[2] * d[3] + g[2] * g[3]) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

__global__ __launch_bounds__(256) void k_eval_iou_groups(int mode3d, int n_groups, const int* __restrict__ dt_off,
                                                         const int* __restrict__ gt_off, const int64_t* __restrict__ iou_off,
                                                         const double* __restrict__ dt_bbox, const double* __restrict__ gt_bbox,
                                                         const float* __restrict__ dt_box3d, const float* __restrict__ gt_box3d,
                                                         double prox_thresh, double* __restrict__ iou,
                                                         unsigned char* __restrict__ prox, int* __restrict__ nonfinite) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= iou_off[n_groups]) return;
    // the group of this pair: the last g with iou_off[g] <= idx (groups without pairs repeat an offset and are skipped)
    int lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (iou_off[mid] <= idx) lo = mid; else hi = mid;
    }
    const int g = lo, G = gt_off[g + 1] - gt_off[g];
    const int64_t r = idx - iou_off[g];
    const int64_t di = dt_off[g] + r / G, gi = gt_off[g] + r % G;
    double v;
    if (mode3d) {
        float vol, u;
        iou3d_pair(dt_box3d + di * 24, gt_box3d + gi * 24, &vol, &u);
        v = (double)u;
    } else {
        v = iou_xywh_pair(dt_bbox + di * 4, gt_bbox + gi * 4);
    }
    iou[idx] = v;
    if (prox) prox[idx] = iou_xywh_pair(dt_bbox + di * 4, gt_bbox + gi * 4) > prox_thresh;
    if (!(fabs(v) <= 1.7976931348623157e308)) nonfinite[g] = 1;       // every writer stores the same value: no atomic
}

// (tier, IoU, index) of a candidate: tier 1 a real ground truth, 0 an ignored one, -1 none.  The larger key wins; equal
// IoUs inside a tier go to the larger index, which is the last one of the host's scan.
struct MatchKey { int tier; double iou; int idx; };
__device__ __forceinline__ bool key_less(const MatchKey& a, const MatchKey& b) {
    if (a.tier != b.tier) return a.tier < b.tier;
    if (a.iou != b.iou) return a.iou < b.iou;
    return a.idx < b.idx;
}

// One workgroup per group, one wave per range.  Lane l owns the ground truths l, l + 64, ...: it alone reads and writes
// their gt_match entries, so the sequential scan over detections needs no barrier.
__global__ __launch_bounds__(256) void k_eval_match_groups(const int* __restrict__ dt_off, const int* __restrict__ gt_off,
                                                           const int64_t* __restrict__ iou_off, const double* __restrict__ iou,
                                                           const unsigned char* __restrict__ prox,
                                                           const double* __restrict__ dt_val, const double* __restrict__ gt_val,
                                                           const unsigned char* __restrict__ gt_flag,
                                                           const double* __restrict__ rng, const double* __restrict__ thrs, int T,
                                                           int* __restrict__ match, unsigned char* __restrict__ dt_ignore,
                                                           unsigned char* __restrict__ gt_ignore, int* __restrict__ gt_match) {
    const int g = blockIdx.x, a = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int d0 = dt_off[g], g0 = gt_off[g];
    const int D = dt_off[g + 1] - d0, G = gt_off[g + 1] - g0;
    const double lo = rng[2 * a], hi = rng[2 * a + 1];
    const double* __restrict__ iou_g = iou + iou_off[g];
    const unsigned char* __restrict__ prox_g = prox ? prox + iou_off[g] : nullptr;
    // outputs of group g: 4 ranges x T x D (match, dt_ignore), 4 x G (gt_ignore), 4 x T x G (gt_match)
    int* __restrict__ m_out = match + ((int64_t)4 * d0 + (int64_t)a * D) * T;
    unsigned char* __restrict__ di_out = dt_ignore + ((int64_t)4 * d0 + (int64_t)a * D) * T;
    unsigned char* __restrict__ gi_out = gt_ignore + (int64_t)4 * g0 + (int64_t)a * G;
    int* __restrict__ gm_out = gt_match + ((int64_t)4 * g0 + (int64_t)a * G) * T;

    for (int gi = lane; gi < G; gi += 64) {
        const double v = gt_val[g0 + gi];
        gi_out[gi] = (gt_flag[g0 + gi] != 0) || v < lo || v > hi;
    }
    for (int t = 0; t < T; ++t) {
        const double thr = fmin(thrs[t], 1.0 - 1e-10);
        int* __restrict__ gm = gm_out + (int64_t)t * G;
        for (int gi = lane; gi < G; gi += 64) gm[gi] = -1;
        for (int d = 0; d < D; ++d) {
            MatchKey best{-1, 0.0, -1};
            bool near = false;
            for (int gi = lane; gi < G; gi += 64) {
                const bool px = prox_g ? prox_g[(int64_t)d * G + gi] != 0 : true;
                near |= px;
                const double v = iou_g[(int64_t)d * G + gi];
                if (px && gm[gi] < 0 && v >= thr) {
                    const MatchKey k{gi_out[gi] ? 0 : 1, v, gi};
                    if (key_less(best, k)) best = k;
                }
            }
            for (int s = 32; s > 0; s >>= 1) {
                const MatchKey o{__shfl_xor(best.tier, s, 64), __shfl_xor(best.iou, s, 64), __shfl_xor(best.idx, s, 64)};
                if (key_less(best, o)) best = o;
            }
            const bool any_near = __ballot(near) != 0ull;
            if (best.tier >= 0 && (best.idx & 63) == lane) gm[best.idx] = d;
            if (lane == 0) {
                const double v = dt_val[d0 + d];
                m_out[(int64_t)t * D + d] = best.idx;
                di_out[(int64_t)t * D + d] = best.tier >= 0 ? best.tier == 0 : ((v < lo || v > hi) || (prox_g && G > 0 && !any_near));
            }
        }
    }
}

extern "C" int cr_eval_iou_groups(cr_ctx* ctx, int mode3d, int n_groups, const int* dt_off, const int* gt_off,
                                  const int64_t* iou_off, int64_t n_pairs, const double* dt_bbox, const double* gt_bbox,
                                  const float* dt_box3d, const float* gt_box3d, double prox_thresh, double* iou,
                                  unsigned char* prox, int* nonfinite) {
    CR_CHECK_ARG(ctx && n_groups >= 0 && n_pairs >= 0, "cr_eval_iou_groups: bad args");
    if (n_groups == 0) return CR_OK;
    CR_CHECK_ARG(dt_off && gt_off && iou_off && nonfinite, "cr_eval_iou_groups: NULL pointer");
    CR_HIP(hipMemsetAsync(nonfinite, 0, sizeof(int) * (size_t)n_groups, ctx->stream));
    if (n_pairs == 0) return CR_OK;
    CR_CHECK_ARG(iou && (mode3d ? (dt_box3d && gt_box3d) : (dt_bbox && gt_bbox)) && (!prox || (dt_bbox && gt_bbox)),
                 "cr_eval_iou_groups: NULL pointer");
    CR_CHECK_ARG(cr_cdiv(n_pairs, 256) <= 0x7fffffff, "cr_eval_iou_groups: too many pairs for one launch");
    hipLaunchKernelGGL(k_eval_iou_groups, dim3((unsigned)cr_cdiv(n_pairs, 256)), dim3(256), 0, ctx->stream, mode3d, n_groups,
                       dt_off, gt_off, iou_off, dt_bbox, gt_bbox, dt_box3d, gt_box3d, prox_thresh, iou, prox, nonfinite);
    CR_LAUNCH_CHECK();
    return CR_OK;
}

extern "C" int cr_eval_match_groups(cr_ctx* ctx, int n_groups, const int* dt_off, const int* gt_off, const int64_t* iou_off,
                                    const double* iou, const unsigned char* prox, const double* dt_val, const double* gt_val,
                                    const unsigned char* gt_flag, const double* rng, const double* thrs, int T, int* match,
                                    unsigned char* dt_ignore, unsigned char* gt_ignore, int* gt_match) {
    CR_CHECK_ARG(ctx && n_groups >= 0 && T >= 0, "cr_eval_match_groups: bad args");
    if (n_groups == 0) return CR_OK;
    CR_CHECK_ARG(dt_off && gt_off && iou_off && rng && (T == 0 || thrs), "cr_eval_match_groups: NULL pointer");
    hipLaunchKernelGGL(k_eval_match_groups, dim3((unsigned)n_groups), dim3(256), 0, ctx->stream, dt_off, gt_off, iou_off, iou,
                       prox, dt_val, gt_val, gt_flag, rng, thrs, T, match, dt_ignore, gt_ignore, gt_match);
    CR_LAUNCH_CHECK();
    return CR_OK;
}
