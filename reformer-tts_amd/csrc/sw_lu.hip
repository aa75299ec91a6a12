// SqueezeWave training: the invertible 1x1 convolutions factored on the device (include/rtts.h: rtts_sw_inv1x1_factor).
//
// Replaces torch.logdet(W) and W.inverse() of the reference's InvertibleConv1d (squeeze_wave/modules.py:63, :79) for ALL flows
// of a model in one launch, in float64, so that a training step never touches the host.
//
// One workgroup owns one matrix.  W (n x n fp32, n <= 128) is widened to float64 into LDS (row stride n | 1 doubles: a column
// walk then touches every bank pair once) and inverted IN PLACE by Gauss-Jordan elimination with partial (row) pivoting:
//
//   step k   p = the row in [k, n) with the largest |a[.][k]|, the LOWEST index on a tie; pivot = a[p][k]
//            rows k and p change places; row k <- row k / pivot with 1 / pivot in column k;
//            row i <- row i - a[i][k] * row k for every other i, column k taken as 0 before the update
//
// which leaves R = (P W)^-1 = W^-1 P^T; the row permutation is undone on the way out (W^-1[i][perm[r]] = R[i][r]) and W^-1 is
// rounded to fp32 once, at the store.  log|det W| = sum_k log|pivot_k| (float64, in pivot order), sign = parity * prod sign(pivot_k).
// A pivot that is exactly 0 ends the elimination: sign 0, log|det| = -inf, W^-1 all NaN.
//
// Every wave finds the pivot and scales the pivot row for itself from the same LDS words (a 64-lane butterfly with a total
// order on (|a|, row), the result taken from lane 0), so a step costs two barriers: one between its reads and its writes, one
// at its end.  Nothing depends on the other matrices of the launch: a matrix comes out bit for bit the same alone and in any
// batch.  No atomics.
#include "rtts_common.h"

#include <math.h>

#define SWLU_THREADS 512
#define SWLU_WAVES (SWLU_THREADS / 64)
#define SWLU_MAX_N RTTS_SW_FACTOR_MAX_N
#define SWLU_MAX_COUNT RTTS_SW_FACTOR_MAX_COUNT

struct SwLuArgs {                       // by value in the kernel's argument block: a captured graph carries the addresses itself
    const float* w[SWLU_MAX_COUNT];
    float* winv[SWLU_MAX_COUNT];
    int n[SWLU_MAX_COUNT];
};

static inline size_t swlu_lds_bytes(int n) { return (size_t)n * (n | 1) * sizeof(double) + 2 * SWLU_MAX_N * sizeof(int); }

__global__ __launch_bounds__(SWLU_THREADS) void sw_inv1x1_factor_kernel(const SwLuArgs args, double* __restrict__ slogdet) {
    extern __shared__ __attribute__((aligned(16))) double swlu_lds[];
    const int m = blockIdx.x;
    const int n = args.n[m], ld = n | 1;
    const float* __restrict__ w = args.w[m];
    float* __restrict__ winv = args.winv[m];
    double* a = swlu_lds;
    int* perm = reinterpret_cast<int*>(swlu_lds + (size_t)n * ld);      // perm[r] = the row of W that now sits in row r
    int* iperm = perm + SWLU_MAX_N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int e = tid; e < n * n; e += SWLU_THREADS) {
        const int i = e / n, j = e - i * n;
        a[i * ld + j] = (double)w[e];
    }
    if (tid < n) perm[tid] = tid;
    __syncthreads();

    double logabs = 0.0;
    int sign = 1;
    const int j0 = lane, j1 = lane + 64;                                // the (at most two) columns of a lane
    for (int k = 0; k < n; ++k) {
        // ---- pivot: the largest |a[i][k]| over i in [k, n), the lowest row on a tie; every wave for itself
        double best = -1.0;
        int p = 0x7fffffff;
        {
            const int i0 = k + lane, i1 = k + lane + 64;
            if (i0 < n) { best = fabs(a[i0 * ld + k]); p = i0; }
            if (i1 < n) {
                const double v = fabs(a[i1 * ld + k]);
                if (v > best) { best = v; p = i1; }
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double ov = __shfl_xor(best, off, 64);
            const int op = __shfl_xor(p, off, 64);
            if (ov > best || (ov == best && op < p)) { best = ov; p = op; }
        }
        p = __shfl(p, 0, 64);                                           // one answer per wave whatever a NaN did to the order
        if (p < k || p >= n) p = k;
        const double pivot = a[p * ld + k];
        if (pivot == 0.0) { sign = 0; break; }                          // the same LDS word for every thread: a uniform exit
        // ---- reads of this step: the pivot row, the row it changes places with
        const double fk = a[k * ld + k];
        double rk0 = 0.0, rk1 = 0.0, ok0 = 0.0, ok1 = 0.0;
        if (j0 < n) { rk0 = a[p * ld + j0]; ok0 = a[k * ld + j0]; }
        if (j1 < n) { rk1 = a[p * ld + j1]; ok1 = a[k * ld + j1]; }
        logabs += log(fabs(pivot));
        if (pivot < 0.0) sign = -sign;
        if (p != k) sign = -sign;
        const double rs0 = j0 == k ? 1.0 / pivot : rk0 / pivot;
        const double rs1 = j1 == k ? 1.0 / pivot : rk1 / pivot;
        __syncthreads();
        // ---- writes: a wave owns whole rows, so the multiplier a[i][k] is read before its lane of column k overwrites it
        for (int i = wave; i < n; i += SWLU_WAVES) {
            double* row = a + i * ld;
            if (i == k) {
                if (j0 < n) row[j0] = rs0;
                if (j1 < n) row[j1] = rs1;
            } else {
                const bool swapped = i == p;                            // row p receives the old row k, eliminated
                const double f = swapped ? fk : row[k];
                if (j0 < n) {
                    const double src = j0 == k ? 0.0 : (swapped ? ok0 : row[j0]);
                    row[j0] = src - f * rs0;
                }
                if (j1 < n) {
                    const double src = j1 == k ? 0.0 : (swapped ? ok1 : row[j1]);
                    row[j1] = src - f * rs1;
                }
            }
        }
        if (tid == 0 && p != k) {
            const int t = perm[k];
            perm[k] = perm[p];
            perm[p] = t;
        }
        __syncthreads();
    }

    if (sign == 0) {
        const float nan = __int_as_float(0x7fc00000);
        for (int e = tid; e < n * n; e += SWLU_THREADS) winv[e] = nan;
        if (tid == 0) {
            slogdet[2 * m] = 0.0;
            slogdet[2 * m + 1] = -INFINITY;
        }
        return;
    }
    if (tid < n) iperm[perm[tid]] = tid;
    __syncthreads();
    for (int e = tid; e < n * n; e += SWLU_THREADS) {
        const int i = e / n, c = e - i * n;
        winv[e] = (float)a[i * ld + iperm[c]];
    }
    if (tid == 0) {
        slogdet[2 * m] = (double)sign;
        slogdet[2 * m + 1] = logabs;
    }
}

static RttsLdsState g_swlu_lds;

extern "C" int rtts_sw_inv1x1_factor(const float* const* w, const int* n, int count, float* const* winv, double* slogdet, void* stream) {
    RTTS_REQUIRE(count >= 1 && count <= SWLU_MAX_COUNT, "rtts_sw_inv1x1_factor: count must be 1..%d (got %d)", SWLU_MAX_COUNT, count);
    RTTS_REQUIRE(w, "rtts_sw_inv1x1_factor: w is null");
    RTTS_REQUIRE(n, "rtts_sw_inv1x1_factor: n is null");
    RTTS_REQUIRE(winv, "rtts_sw_inv1x1_factor: winv is null");
    RTTS_REQUIRE(slogdet, "rtts_sw_inv1x1_factor: slogdet is null");
    SwLuArgs args = {};
    int nmax = 0;
    for (int i = 0; i < count; ++i) {
        RTTS_REQUIRE(n[i] >= 1 && n[i] <= SWLU_MAX_N, "rtts_sw_inv1x1_factor: n[%d] must be 1..%d (got %d)", i, SWLU_MAX_N, n[i]);
        RTTS_REQUIRE(w[i], "rtts_sw_inv1x1_factor: w[%d] is null", i);
        RTTS_REQUIRE(winv[i], "rtts_sw_inv1x1_factor: winv[%d] is null", i);
        args.w[i] = w[i];
        args.winv[i] = winv[i];
        args.n[i] = n[i];
        nmax = n[i] > nmax ? n[i] : nmax;
    }
    RTTS_ENTER(stream);
    const size_t lds = swlu_lds_bytes(nmax);
    static_assert((size_t)SWLU_MAX_N * (SWLU_MAX_N | 1) * sizeof(double) + 2 * SWLU_MAX_N * sizeof(int) <= 160 * 1024,
                  "the largest matrix in float64 must fit the 160 KB of LDS");
    RTTS_ENSURE_LDS("rtts_sw_inv1x1_factor", sw_inv1x1_factor_kernel, lds, g_swlu_lds);
    hipLaunchKernelGGL(sw_inv1x1_factor_kernel, dim3((unsigned)count), dim3(SWLU_THREADS), lds, (hipStream_t)stream, args, slogdet);
    RTTS_LAUNCH_CHECK("rtts_sw_inv1x1_factor");
    return 0;
}
