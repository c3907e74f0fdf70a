"""GPU: the order of additions of the BatchNorm statistics finalize (cr_bn_fwd on the unfused route), for the single launch
(k_bn_finalize) and the two-launch form for many rows (k_bn_stats_lanes + k_bn_finalize_lanes): mean_invstd, running_mean
and running_var must be BIT-equal to a NumPy float64 emulation of the documented order, which is the specification:

  lane t of 256 adds the rows r = t, t + 256, t + 512, ... ascending, each float32 row value converted to double;
  the 256 lane sums go through the tree  for off in 128, 64, ..., 1: lane[t] += lane[t + off]  (t < off);
  mean = s / count;  var = max(fma(-mean, mean, q / count), 0);  invstd = 1 / sqrt(var + eps);
  unbiased = var * count / (count - 1);  running = fma(momentum, value, (1 - momentum) * running)
  -- all in double, count / eps / momentum being the call's float32 arguments; results rounded to float32 once.

Synthetic statistics rows are fed straight to cr_bn_fwd.  Even channels hold ordinary values, odd channels large sums with a
small variance (mean ~100 - 200, sigma 0.5: the sum of squares exceeds 2^24 times the variance's contribution per row, so a
float32 accumulation would lose it and the double accumulation matters).  Cases: C = 16 with 300 and 1000 rows (not
multiples of 256, single launch), C = 32 with 4096 rows, C = 16 with 2348 rows (two launches, a tail of rows in both the
batched and the row-by-row part of step 1) and the stem's own 16 384 rows."""
import importlib
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
lib = importlib.import_module("3dod_amd._lib")
DEV = torch.device("cuda:0")
EPS, MOMENTUM = np.float32(1e-5), np.float32(0.1)
CASES = [(16, 300), (16, 1000), (32, 4096), (16, 2348), (16, 16384)]


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic; int / int division rounds to nearest even)"""
    return np.float64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def emulate(rows, count, rm, rv):
    """rows: float32 [nparts][2][C] -> (mean_invstd [2][C], running_mean, running_var) as float32"""
    nparts, _, C = rows.shape
    lanes = np.zeros((256, 2, C), np.float64)
    for r0 in range(0, nparts, 256):                       # lane t += row r0 + t, ascending in r0
        blk = rows[r0:r0 + 256].astype(np.float64)
        lanes[:blk.shape[0]] += blk
    off = 128
    while off > 0:
        lanes[:off] += lanes[off:2 * off]
        off >>= 1
    cnt, eps, mom = np.float64(np.float32(count)), np.float64(EPS), np.float64(MOMENTUM)
    mi, rm_new, rv_new = np.empty((2, C), np.float32), np.empty(C, np.float32), np.empty(C, np.float32)
    for c in range(C):
        mean = lanes[0, 0, c] / cnt
        var = fma(-mean, mean, lanes[0, 1, c] / cnt)
        if var < 0.0:
            var = np.float64(0.0)
        mi[0, c] = np.float32(mean)
        mi[1, c] = np.float32(np.float64(1.0) / np.sqrt(var + eps))
        unbiased = var * cnt / (cnt - np.float64(1.0)) if cnt > 1.0 else var
        rm_new[c] = np.float32(fma(mom, mean, (np.float64(1.0) - mom) * np.float64(rm[c])))
        rv_new[c] = np.float32(fma(mom, unbiased, (np.float64(1.0) - mom) * np.float64(rv[c])))
    return mi, rm_new, rv_new


def synthetic_rows(C, nparts, rng):
    mu = np.where(np.arange(C) % 2 == 0, rng.normal(0, 1, C), 100.0 * (1.0 + np.arange(C) / C))
    sigma = np.where(np.arange(C) % 2 == 0, rng.uniform(0.5, 2.0, C), 0.5)
    s = 64 * mu + 8 * sigma * rng.normal(0, 1, (nparts, C))                      # sum of 64 pixels
    q = s * s / 64 + 64 * sigma ** 2 * rng.uniform(0.8, 1.2, (nparts, C))        # their sum of squares (row variance > 0)
    return np.stack([s, q], 1).astype(np.float32)


def test_emulated_fma_rounds_once():
    a, b, c = np.float64(1 + 2.0 ** -30), np.float64(1 - 2.0 ** -30), np.float64(-1.0)
    assert fma(a, b, c) == -2.0 ** -60 and a * b + c == 0.0


@pytest.mark.parametrize("C,nparts", CASES)
def test_finalize_bits(C, nparts):
    rng = np.random.default_rng(100 * C + nparts)
    rows = synthetic_rows(C, nparts, rng)
    M = 64 * nparts                                        # the rows are those of full 64-pixel tiles
    rm = rng.normal(0, 1, C).astype(np.float32)
    rv = rng.uniform(0.5, 2.0, C).astype(np.float32)
    want_mi, want_rm, want_rv = emulate(rows, M, rm, rv)
    assert (want_mi[1, 1::2] < 4.0).all() and (want_mi[1, 1::2] > 1.0).all()    # sigma 0.5 was resolved (1 / sigma = 2)
    x = torch.zeros(M, C, device=DEV)
    y, mi = torch.empty_like(x), torch.empty(2, C, device=DEV)
    rmd, rvd = torch.from_numpy(rm).to(DEV), torch.from_numpy(rv).to(DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    lib.call("cr_bn_fwd", x, torch.from_numpy(rows).to(DEV), nparts, gamma, beta, None, y, M, C, 0, float(EPS), float(MOMENTUM),
             mi, rmd, rvd, 1)
    torch.cuda.synchronize()
    for name, got, want in (("mean_invstd", mi, want_mi), ("running_mean", rmd, want_rm), ("running_var", rvd, want_rv)):
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, got, want)
    # the apply that follows reads those two floats: y = (0 - mean) * invstd
    assert torch.equal(y[0], (0.0 - mi[0]) * mi[1])
