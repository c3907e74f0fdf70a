// Map table of the Winograd F(2x2, 3x3) route: the maps of one call (pyramid levels x images) as consecutive row blocks of
// the transformed planes.  Shared by the transforms (winograd.hip) and the fused product + output kernel (conv.hip).
#pragma once
#include "cr_common.h"

#define WINO_MAX_MAPS 8
struct WinoMap { const float* src; float* dst; const float* acc; int N, H, W, tbase, blk0; };
struct WinoGeo { WinoMap m[WINO_MAX_MAPS]; int n, C, T; };

__device__ __forceinline__ int wino_find(const WinoGeo& g, int blk) {
    int i = 0;
    while (i + 1 < g.n && blk >= g.m[i + 1].blk0) ++i;
    return i;
}

// tbase: first tile (row of the planes) of a map; blk0: its first block when every map gets whole blocks of tpb tiles per
// channel group of 64 * vec channels (the transforms' grids)
static int wino_geo(const char* who, WinoGeo& g, int n, const float* const* srcs, float* const* dsts, const float* const* accs,
                    const int* Ns, const int* Hs, const int* Ws, int C, int64_t T, int tpb, unsigned* blocks, int* vec) {
    CR_CHECK_ARG(n >= 1 && n <= WINO_MAX_MAPS, "%s: 1..%d maps", who, WINO_MAX_MAPS);
    CR_CHECK_ARG(C > 0 && C % 64 == 0, "%s: channels %% 64", who);
    g.n = n; g.C = C; g.T = (int)T;
    const int v = C % 256 == 0 ? 4 : C % 128 == 0 ? 2 : 1;           // floats per lane: 16-byte accesses when the channels allow
    *vec = v;
    int tb = 0, blk = 0;
    for (int i = 0; i < n; ++i) {
        CR_CHECK_ARG(Ns[i] > 0 && Hs[i] > 0 && Ws[i] > 0 && Hs[i] % 2 == 0 && Ws[i] % 2 == 0, "%s: map %d needs even H and W", who, i);
        g.m[i].src = srcs ? srcs[i] : nullptr; g.m[i].dst = dsts ? dsts[i] : nullptr; g.m[i].acc = accs ? accs[i] : nullptr;
        g.m[i].N = Ns[i]; g.m[i].H = Hs[i]; g.m[i].W = Ws[i]; g.m[i].tbase = tb; g.m[i].blk0 = blk;
        tb += Ns[i] * (Hs[i] / 2) * (Ws[i] / 2);
        blk += (int)cr_cdiv((int64_t)Ns[i] * (Hs[i] / 2) * (Ws[i] / 2), tpb) * (C / (64 * v));
    }
    CR_CHECK_ARG(tb == T && (int64_t)T * C * 16 < (1ll << 40), "%s: T = %lld does not match the maps (%d tiles)", who, (long long)T, tb);
    for (int i = n; i < WINO_MAX_MAPS; ++i) g.m[i] = g.m[n - 1];
    *blocks = (unsigned)blk;
    return CR_OK;
}
