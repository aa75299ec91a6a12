// SqueezeWave vocoder, inference path: the pieces between the 1x1-convolution GEMMs of a WN block
// (/root/reference/reformer_tts/squeeze_wave/modules.py:88-122 depthwise separable convolution with its BatchNorm folded,
// :10-24 the tanh*sigmoid gate with the nearest-neighbour upsampled mel conditioning :216-225, :353-359 the inverse of
// the affine coupling).  Activations are channels-last rows (B*L, C) -- a 1x1 Conv1d is then a plain GEMM over rows and
// every kernel here streams rows with 8/16-byte accesses; all three are HBM-bound elementwise/stencil kernels.
#include "rtts_common.h"

#define SW_THREADS 256

static inline unsigned sw_grid(size_t items) {
    size_t b = (items + SW_THREADS - 1) / SW_THREADS;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// Segments of packed rows (SqueezeWave.infer_ragged): utterances laid end to end, segment s = mel frames [moff[s], moff[s+1])
// of a device int32 table of nseg + 1 non-decreasing offsets, audio rows [up * moff[s], up * moff[s+1]).  The table is read
// when the kernel runs (a replayed hipGraph takes new lengths); at most SW_MAX_SEGMENTS segments (it is staged in LDS).
#define SW_MAX_SEGMENTS 1024

// [a, e) = the rows of the segment that holds `row`: between the largest row offset <= row and the next one.  Rows before
// up * moff[0] and from up * moff[nseg] on (the capacity padding) form segments of their own.  The bracket is clamped to
// [0, rows) and around `row`, so even a malformed table never sends a read outside the buffer.
__device__ __forceinline__ void sw_segment_of(long long row, const int* s_off, int nseg, int up, long long rows, long long& a, long long& e) {
    int lo = 0, hi = nseg + 1;                         // upper bound: the first offset above row
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)up * s_off[mid] <= row) lo = mid + 1;
        else hi = mid;
    }
    a = lo > 0 ? (long long)up * s_off[lo - 1] : 0;
    e = lo <= nseg ? (long long)up * s_off[lo] : rows;
    a = a < 0 ? 0 : (a > row ? row : a);
    e = e > rows ? rows : (e <= row ? row + 1 : e);
}

// y[b][l][c] = bias[c] + sum_k w[c][k] * x[b][l + k - 1][c]   (kernel 3, zero padding), x fp32 -> y bf16; 4 channels/thread.
// edge_lo / edge_hi (may be null): per-channel constants subtracted at l = 0 / l = L-1 -- with an eval-mode BatchNorm folded
// into w and bias, the reference's zero padding pads bn(x), so the folded constant must not be counted for the missing tap.
// SEG = false: B sequences of L rows (moff unused); SEG = true: the segments of the offset table moff (L unused), each with
// its own zero padding and edge corrections.  Both read and compute exactly the same taps for a row of the same sequence.
template <bool SEG>
__global__ __launch_bounds__(SW_THREADS) void sw_depthwise_k3_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, int L, int C, size_t n4,
                                                                     bf16_t* __restrict__ y, const float* __restrict__ edge_lo,
                                                                     const float* __restrict__ edge_hi, const int* __restrict__ moff,
                                                                     int nseg, int up) {
    const int c4 = C / 4;
    __shared__ int s_off[SEG ? SW_MAX_SEGMENTS + 1 : 1];
    if (SEG) {
        for (int i = threadIdx.x; i <= nseg; i += blockDim.x) s_off[i] = moff[i];
        __syncthreads();
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4) * 4;
        const size_t row = i / c4;
        bool first, last;
        if (SEG) {
            long long a, e;
            sw_segment_of((long long)row, s_off, nseg, up, (long long)(n4 / c4), a, e);
            first = (long long)row == a;
            last = (long long)row + 1 == e;
        } else {
            const int l = (int)(row % L);
            first = l == 0;
            last = l + 1 == L;
        }
        const float4 mid = *reinterpret_cast<const float4*>(x + row * C + c);
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (!first) lo = *reinterpret_cast<const float4*>(x + (row - 1) * C + c);
        if (!last) hi = *reinterpret_cast<const float4*>(x + (row + 1) * C + c);
        const float a[4] = {lo.x, lo.y, lo.z, lo.w}, m[4] = {mid.x, mid.y, mid.z, mid.w}, h[4] = {hi.x, hi.y, hi.z, hi.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* wc = w + (size_t)(c + j) * 3;
            o[j] = __builtin_fmaf(wc[0], a[j], __builtin_fmaf(wc[1], m[j], __builtin_fmaf(wc[2], h[j], bias[c + j])));
            if (edge_lo && first) o[j] -= edge_lo[c + j];
            if (edge_hi && last) o[j] -= edge_hi[c + j];
        }
        uint2 pk;
        pk.x = pack_bf16x2(o[0], o[1]);
        pk.y = pack_bf16x2(o[2], o[3]);
        *reinterpret_cast<uint2*>(y + row * C + c) = pk;
    }
}

// acts[m][c] = tanh(pw[m][c] + cond[r][off + c]) * sigmoid(pw[m][C + c] + cond[r][off + C + c]),  r = (b, l / up):
// the per-layer slice of the mel conditioning, nearest-neighbour upsampled; 8 channels per thread.  Packed rows need no
// table here: audio row m of segment s reads moff[s] + (m - up * moff[s]) / up = m / up, the B = 1 case over all rows.
__global__ __launch_bounds__(SW_THREADS) void sw_gate_kernel(const bf16_t* __restrict__ pw, const bf16_t* __restrict__ cond, int64_t ld_cond,
                                                             int off, int up, int L, int Lm, int C, size_t n8, bf16_t* __restrict__ acts) {
    const int c8 = C / 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c8) * 8;
        const size_t row = i / c8;
        const size_t b = row / L;
        const int l = (int)(row % L);
        const size_t crow = b * Lm + (up > 1 ? l / up : l);
        const uint4 pt = *reinterpret_cast<const uint4*>(pw + row * 2 * C + c);
        const uint4 ps = *reinterpret_cast<const uint4*>(pw + row * 2 * C + C + c);
        const uint4 ct = *reinterpret_cast<const uint4*>(cond + crow * ld_cond + off + c);
        const uint4 cs = *reinterpret_cast<const uint4*>(cond + crow * ld_cond + off + C + c);
        const uint32_t a[4] = {pt.x, pt.y, pt.z, pt.w}, bq[4] = {ps.x, ps.y, ps.z, ps.w};
        const uint32_t e[4] = {ct.x, ct.y, ct.z, ct.w}, f[4] = {cs.x, cs.y, cs.z, cs.w};
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t0 = __uint_as_float(a[j] << 16) + __uint_as_float(e[j] << 16);
            const float t1 = __uint_as_float(a[j] & 0xffff0000u) + __uint_as_float(e[j] & 0xffff0000u);
            const float s0 = __uint_as_float(bq[j] << 16) + __uint_as_float(f[j] << 16);
            const float s1 = __uint_as_float(bq[j] & 0xffff0000u) + __uint_as_float(f[j] & 0xffff0000u);
            o[j] = pack_bf16x2(tanhf(t0) / (1.f + __expf(-s0)), tanhf(t1) / (1.f + __expf(-s1)));
        }
        *reinterpret_cast<uint4*>(acts + row * C + c) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// Packed mel rows for the ragged vocoder: dst[r][c] (fp32, row stride ld_dst) = mel[s][c][r - moff[s]] for the frames r of
// segment s, zero in every other row up to `rows` (the capacity) and wherever the source frame would lie past L.  mel is read
// through its three element strides (any layout of (B, n_mel, L)); one thread per output element, channels fastest.
__global__ __launch_bounds__(SW_THREADS) void sw_pack_mel_kernel(const float* __restrict__ mel, int64_t sb, int64_t sc, int64_t st, int L,
                                                                 int n_mel, const int* __restrict__ moff, int nseg, long long rows,
                                                                 float* __restrict__ dst, int64_t ld_dst) {
    __shared__ int s_off[SW_MAX_SEGMENTS + 1];
    for (int i = threadIdx.x; i <= nseg; i += blockDim.x) s_off[i] = moff[i];
    __syncthreads();
    const size_t n = (size_t)rows * n_mel;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const long long r = (long long)(i / n_mel);
        const int c = (int)(i % n_mel);
        int lo = 0, hi = nseg + 1;                     // s = (first offset above r) - 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= r) lo = mid + 1;
            else hi = mid;
        }
        const int s = lo - 1;
        float v = 0.f;
        if (s >= 0 && s < nseg && r < s_off[s + 1]) {
            const long long t = r - s_off[s];
            if (t < L) v = mel[(int64_t)s * sb + (int64_t)c * sc + t * st];
        }
        dst[r * ld_dst + c] = v;
    }
}

// inverse affine coupling, in place on the second half of the channels: a1 = (a1 - b) / exp(s), wn = [s | b] (fp32)
__global__ __launch_bounds__(SW_THREADS) void sw_coupling_inv_kernel(float* __restrict__ audio, int64_t ld_audio, const float* __restrict__ wn,
                                                                     int half, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / half;
        const int c = (int)(i % half);
        float* a1 = audio + row * ld_audio + half + c;
        const float s = wn[row * 2 * half + c], b = wn[row * 2 * half + half + c];
        *a1 = (*a1 - b) * __expf(-s);
    }
}

extern "C" int rtts_sw_depthwise_k3(const float* x, const float* w, const float* bias, int B, int L, int C, void* y, const float* edge_lo,
                                    const float* edge_hi, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(x && w && bias && y && B > 0 && L > 0 && C > 0 && C % 4 == 0, "rtts_sw_depthwise_k3: bad arguments (C %% 4 == 0)");
    const size_t n4 = (size_t)B * L * C / 4;
    hipLaunchKernelGGL(sw_depthwise_k3_kernel<false>, dim3(sw_grid(n4)), dim3(SW_THREADS), 0, (hipStream_t)stream, x, w, bias, L, C, n4, (bf16_t*)y,
                       edge_lo, edge_hi, (const int*)nullptr, 0, 1);
    RTTS_LAUNCH_CHECK("rtts_sw_depthwise_k3");
    return 0;
}

extern "C" int rtts_sw_depthwise_k3_seg(const float* x, const float* w, const float* bias, const int32_t* moff, int nseg, int upsample,
                                        int64_t rows, int C, void* y, const float* edge_lo, const float* edge_hi, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(x && w && bias && y && moff && rows > 0 && C > 0 && C % 4 == 0 && upsample >= 1 && rows % upsample == 0,
                 "rtts_sw_depthwise_k3_seg: bad arguments (C %% 4 == 0, rows a multiple of upsample)");
    RTTS_REQUIRE(nseg >= 1 && nseg <= SW_MAX_SEGMENTS, "rtts_sw_depthwise_k3_seg: 1..%d segments (got %d)", SW_MAX_SEGMENTS, nseg);
    const size_t n4 = (size_t)rows * C / 4;
    hipLaunchKernelGGL(sw_depthwise_k3_kernel<true>, dim3(sw_grid(n4)), dim3(SW_THREADS), 0, (hipStream_t)stream, x, w, bias, 0, C, n4, (bf16_t*)y,
                       edge_lo, edge_hi, (const int*)moff, nseg, upsample);
    RTTS_LAUNCH_CHECK("rtts_sw_depthwise_k3_seg");
    return 0;
}

extern "C" int rtts_sw_gate(const void* pw, const void* cond, int64_t ld_cond, int cond_offset, int upsample, int B, int L, int Lm, int C,
                            void* acts, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(pw && cond && acts && B > 0 && L > 0 && Lm > 0 && C > 0 && C % 8 == 0 && cond_offset % 8 == 0 && ld_cond % 8 == 0 &&
                     upsample >= 1 && (int64_t)Lm * upsample == L && ld_cond >= cond_offset + 2 * C,
                 "rtts_sw_gate: bad arguments (C %% 8 == 0, L == Lm * upsample)");
    const size_t n8 = (size_t)B * L * C / 8;
    hipLaunchKernelGGL(sw_gate_kernel, dim3(sw_grid(n8)), dim3(SW_THREADS), 0, (hipStream_t)stream, (const bf16_t*)pw, (const bf16_t*)cond,
                       ld_cond, cond_offset, upsample, L, Lm, C, n8, (bf16_t*)acts);
    RTTS_LAUNCH_CHECK("rtts_sw_gate");
    return 0;
}

extern "C" int rtts_sw_pack_mel(const float* mel, int64_t stride_b, int64_t stride_c, int64_t stride_t, int L, int n_mel, const int32_t* moff,
                                int nseg, int64_t rows, float* dst, int64_t ld_dst, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(mel && moff && dst && L >= 0 && n_mel > 0 && rows > 0 && ld_dst >= n_mel, "rtts_sw_pack_mel: bad arguments");
    RTTS_REQUIRE(nseg >= 1 && nseg <= SW_MAX_SEGMENTS, "rtts_sw_pack_mel: 1..%d segments (got %d)", SW_MAX_SEGMENTS, nseg);
    const size_t n = (size_t)rows * n_mel;
    hipLaunchKernelGGL(sw_pack_mel_kernel, dim3(sw_grid(n)), dim3(SW_THREADS), 0, (hipStream_t)stream, mel, stride_b, stride_c, stride_t, L, n_mel,
                       (const int*)moff, nseg, (long long)rows, dst, ld_dst);
    RTTS_LAUNCH_CHECK("rtts_sw_pack_mel");
    return 0;
}

extern "C" int rtts_sw_coupling_inv(float* audio, int64_t ld_audio, const float* wn_out, int64_t rows, int half, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(audio && wn_out && rows > 0 && half > 0 && ld_audio >= 2 * half, "rtts_sw_coupling_inv: bad arguments");
    const size_t n = (size_t)rows * half;
    hipLaunchKernelGGL(sw_coupling_inv_kernel, dim3(sw_grid(n)), dim3(SW_THREADS), 0, (hipStream_t)stream, audio, ld_audio, wn_out, half, n);
    RTTS_LAUNCH_CHECK("rtts_sw_coupling_inv");
    return 0;
}

// ------------------------------------------------------------------ inverse coupling + inverse invertible 1x1 convolution
// out (rows, n) fp32 = [a0 | (a1 - b) * exp(-s)] @ Winv^T  -- the tail of one flow of SqueezeWave.infer
// (/root/reference/reformer_tts/squeeze_wave/modules.py:353-361: the affine coupling undone, then InvertibleConv1d's
// W_inverse, :57-85).  The audio path stays fp32 end to end (twelve chained matrix products: bf16 operands would leave ~3
// digits), so this is an fp32 FMA kernel, not an MFMA one: n <= 128 channels, 2*n*n FLOP per row -- 0.4 GFLOP for a
// 2-second utterance.  One workgroup = 32 rows; Winv^T (n x n) and the 32 coupled rows sit in LDS, thread (row, g) owns
// the output columns g, g + 8, ... of its row: the W reads of 8 neighbouring lanes are 8 consecutive words, the x reads
// broadcast.
#define SWI_ROWS 32
#define SWI_MAXN 128
__global__ __launch_bounds__(SW_THREADS) void sw_coupling_inv1x1_kernel(const float* __restrict__ audio, int64_t ld_audio,
                                                                        const float* __restrict__ wn, int64_t ld_wn,
                                                                        const float* __restrict__ winv, int n, int half, long long rows,
                                                                        float* __restrict__ out, int64_t ld_out) {
    extern __shared__ __attribute__((aligned(16))) float swi_smem[];
    float* Wt = swi_smem;                     // [n][n]: Wt[k][c] = Winv[c][k]
    float* X = Wt + n * n;                    // [SWI_ROWS][n + 1]
    const int tid = threadIdx.x;
    for (int i = tid; i < n * n; i += SW_THREADS) {
        const int c = i / n, k = i % n;       // coalesced read of Winv's rows; the transposed store is n-strided (once per block)
        Wt[k * n + c] = winv[i];
    }
    const long long r0 = (long long)blockIdx.x * SWI_ROWS;
    for (int i = tid; i < SWI_ROWS * n; i += SW_THREADS) {
        const int rr = i / n, k = i % n;
        const long long row = r0 + rr;
        float v = 0.f;
        if (row < rows) {
            v = audio[row * ld_audio + k];
            if (k >= half) {
                const float s = wn[row * ld_wn + (k - half)], b = wn[row * ld_wn + k];
                v = (v - b) * __expf(-s);
            }
        }
        X[rr * (n + 1) + k] = v;
    }
    __syncthreads();
    const int rr = tid >> 3, g = tid & 7;
    float acc[SWI_MAXN / 8];
#pragma unroll
    for (int j = 0; j < SWI_MAXN / 8; ++j) acc[j] = 0.f;
    const float* xr = X + rr * (n + 1);
    for (int k = 0; k < n; ++k) {
        const float xv = xr[k];
        const float* wk = Wt + k * n + g;
#pragma unroll
        for (int j = 0; j < SWI_MAXN / 8; ++j)
            if (g + 8 * j < n) acc[j] = __builtin_fmaf(xv, wk[8 * j], acc[j]);
    }
    const long long row = r0 + rr;
    if (row < rows) {
#pragma unroll
        for (int j = 0; j < SWI_MAXN / 8; ++j)
            if (g + 8 * j < n) out[row * ld_out + g + 8 * j] = acc[j];
    }
}

static RttsLdsState g_swi_lds;

extern "C" int rtts_sw_coupling_inv1x1(const float* audio, int64_t ld_audio, const float* wn_out, int64_t ld_wn, const float* winv, int n,
                                       int64_t rows, float* out, int64_t ld_out, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(audio && wn_out && winv && out && rows > 0 && n >= 2 && n % 2 == 0 && n <= SWI_MAXN && ld_audio >= n && ld_wn >= n && ld_out >= n,
                 "rtts_sw_coupling_inv1x1: n must be even and <= %d, leading dimensions >= n (got n=%d)", SWI_MAXN, n);
    RTTS_REQUIRE(out != audio, "rtts_sw_coupling_inv1x1: not in place (a block reads rows of audio that another may have rewritten)");
    const size_t lds = ((size_t)n * n + (size_t)SWI_ROWS * (n + 1)) * sizeof(float);
    RTTS_ENSURE_LDS("rtts_sw_coupling_inv1x1", sw_coupling_inv1x1_kernel, lds, g_swi_lds);
    const unsigned blocks = (unsigned)((rows + SWI_ROWS - 1) / SWI_ROWS);
    hipLaunchKernelGGL(sw_coupling_inv1x1_kernel, dim3(blocks), dim3(SW_THREADS), lds, (hipStream_t)stream, audio, ld_audio, wn_out, ld_wn, winv,
                       n, n / 2, (long long)rows, out, ld_out);
    RTTS_LAUNCH_CHECK("rtts_sw_coupling_inv1x1");
    return 0;
}

// ------------------------------------------------------------------ forward (analysis) direction: audio -> latent z
// One flow boundary of SqueezeWave.forward (reference reformer_tts/squeeze_wave/modules.py:311-328), the mirror of the
// kernel above: the PREVIOUS flow's affine coupling c = [x0 | exp(log_s) * x1 + b] (:326-327), this flow's early output
// (:312-314: the first n_early columns of c go to z at column z_col) and this flow's invertible 1x1 convolution (:53-65,
// y[c] = sum_k W[c][k] x[k]) over the remaining n = n_in - n_early columns, in one fp32 launch.  wn == null: the first flow
// (no coupling in front of it); w == null: the tail after the last flow (n_early == n_in, everything goes to z).
// Same shape as the inverse kernel: 32 rows per workgroup, W^T and the coupled rows in LDS, thread (row, g) owns the output
// columns g, g + 8, ...  The eight lanes of a row also sum its log_s (columns g, g + 8, ... in order, then the fixed DPP
// tree of rtts_sum8): one workgroup owns a row's sum, no atomics, and the order does not depend on where the row falls in a
// workgroup.  ls_row[row] += that sum.
__global__ __launch_bounds__(SW_THREADS) void sw_coupling_fwd1x1_kernel(const float* __restrict__ x, int64_t ld_x,
                                                                        const float* __restrict__ wn, int64_t ld_wn,
                                                                        const float* __restrict__ w, int n_in, int n_early, long long rows,
                                                                        float* __restrict__ out, int64_t ld_out, float* __restrict__ z,
                                                                        int64_t ld_z, int z_col, float* __restrict__ ls_row) {
    extern __shared__ __attribute__((aligned(16))) float swf_smem[];
    const int n = n_in - n_early, half = n_in / 2;
    float* Wt = swf_smem;                     // [n][n]: Wt[k][c] = W[c][k]
    float* X = Wt + n * n;                    // [SWI_ROWS][n_in + 1]: the coupled rows
    const int tid = threadIdx.x;
    if (w) {
        for (int i = tid; i < n * n; i += SW_THREADS) {
            const int c = i / n, k = i % n;
            Wt[k * n + c] = w[i];
        }
    }
    const long long r0 = (long long)blockIdx.x * SWI_ROWS;
    for (int i = tid; i < SWI_ROWS * n_in; i += SW_THREADS) {
        const int rr = i / n_in, k = i % n_in;
        const long long row = r0 + rr;
        float v = 0.f;
        if (row < rows) {
            v = x[row * ld_x + k];
            if (wn && k >= half) {
                const float s = wn[row * ld_wn + (k - half)], b = wn[row * ld_wn + k];
                v = __builtin_fmaf(__expf(s), v, b);
            }
        }
        X[rr * (n_in + 1) + k] = v;
    }
    __syncthreads();
    const int rr = tid >> 3, g = tid & 7;
    const long long row = r0 + rr;
    const float* xr = X + rr * (n_in + 1);
    if (row < rows) {
        for (int k = g; k < n_early; k += 8) z[row * ld_z + z_col + k] = xr[k];
    }
    if (wn) {                                 // all 64 lanes of a wave take part in the DPP sum: rows past the end add zeros
        float ls = 0.f;
        if (row < rows) {
            for (int k = g; k < half; k += 8) ls += wn[row * ld_wn + k];
        }
        ls = rtts_sum8(ls);
        if (row < rows && g == 0) ls_row[row] += ls;
    }
    if (!w) return;
    float acc[SWI_MAXN / 8];
#pragma unroll
    for (int j = 0; j < SWI_MAXN / 8; ++j) acc[j] = 0.f;
    xr += n_early;
    for (int k = 0; k < n; ++k) {
        const float xv = xr[k];
        const float* wk = Wt + k * n + g;
#pragma unroll
        for (int j = 0; j < SWI_MAXN / 8; ++j)
            if (g + 8 * j < n) acc[j] = __builtin_fmaf(xv, wk[8 * j], acc[j]);
    }
    if (row < rows) {
#pragma unroll
        for (int j = 0; j < SWI_MAXN / 8; ++j)
            if (g + 8 * j < n) out[row * ld_out + g + 8 * j] = acc[j];
    }
}

static RttsLdsState g_swf_lds;

extern "C" int rtts_sw_coupling_fwd1x1(const float* x, int64_t ld_x, const float* wn_out, int64_t ld_wn, const float* w, int n_in, int n_early,
                                       int64_t rows, float* out, int64_t ld_out, float* z, int64_t ld_z, int z_col, float* ls_row,
                                       void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(n_in >= 2 && n_in % 2 == 0 && n_in <= SWI_MAXN, "rtts_sw_coupling_fwd1x1: n_in must be even and <= %d (got n_in=%d)", SWI_MAXN,
                 n_in);
    RTTS_REQUIRE(n_early >= 0 && n_early <= n_in && n_early % 2 == 0,
                 "rtts_sw_coupling_fwd1x1: n_early must be even and within [0, n_in] (got n_early=%d, n_in=%d)", n_early, n_in);
    const int n = n_in - n_early;
    RTTS_REQUIRE(x && rows > 0 && ld_x >= n_in && (!wn_out || (ld_wn >= n_in && ls_row)),
                 "rtts_sw_coupling_fwd1x1: bad arguments (x, rows > 0, leading dimensions >= n_in, ls_row with wn_out)");
    RTTS_REQUIRE(n_early == 0 || (z && z_col >= 0 && ld_z >= (int64_t)z_col + n_early),
                 "rtts_sw_coupling_fwd1x1: the early output needs z with ld_z >= z_col + n_early (got z_col=%d, n_early=%d)", z_col, n_early);
    if (w) {
        RTTS_REQUIRE(n >= 2 && out && ld_out >= n, "rtts_sw_coupling_fwd1x1: the convolution needs n = n_in - n_early >= 2 and out with ld_out >= n");
        RTTS_REQUIRE(out != x, "rtts_sw_coupling_fwd1x1: not in place (a block reads rows of x that another may have rewritten)");
    } else {
        RTTS_REQUIRE(n == 0, "rtts_sw_coupling_fwd1x1: without W every column is early output: n_early must equal n_in (got %d, %d)", n_early, n_in);
    }
    RTTS_REQUIRE(!z || (z != x && z != out), "rtts_sw_coupling_fwd1x1: z must not alias x or out");
    const size_t lds = ((size_t)n * n + (size_t)SWI_ROWS * (n_in + 1)) * sizeof(float);
    RTTS_ENSURE_LDS("rtts_sw_coupling_fwd1x1", sw_coupling_fwd1x1_kernel, lds, g_swf_lds);
    const unsigned blocks = (unsigned)((rows + SWI_ROWS - 1) / SWI_ROWS);
    hipLaunchKernelGGL(sw_coupling_fwd1x1_kernel, dim3(blocks), dim3(SW_THREADS), lds, (hipStream_t)stream, x, ld_x, wn_out, ld_wn, w, n_in,
                       n_early, (long long)rows, out, ld_out, z, ld_z, z_col, ls_row);
    RTTS_LAUNCH_CHECK("rtts_sw_coupling_fwd1x1");
    return 0;
}

// Per-utterance sums of the negative log-likelihood (reference reformer_tts/squeeze_wave/loss.py:21-28): out[s] =
// {sum z^2, sum log_s} over the rows of segment s, in float64.  Segment s = audio rows [up * moff[s], up * moff[s+1]) of the
// offset table (clamped to [0, rows), like sw_segment_of: a malformed table cannot send a read outside the buffers), or rows
// [s * L, (s + 1) * L) when moff is null.  One workgroup per segment: thread t adds elements t, t + 256, ... of the segment
// (counted from ITS first row) in order, then a fixed LDS tree -- a segment's sums depend on its rows only, not on where
// they lie.  Rows outside every segment (capacity padding, rows before moff[0]) are never read; an empty segment gives zeros.
__global__ __launch_bounds__(SW_THREADS) void sw_nll_reduce_kernel(const float* __restrict__ z, int64_t ld_z, int C,
                                                                   const float* __restrict__ ls_row, const int* __restrict__ moff, int up,
                                                                   long long L, long long rows, double* __restrict__ out) {
    __shared__ double s_sq[SW_THREADS], s_ls[SW_THREADS];
    const int s = blockIdx.x, tid = threadIdx.x;
    long long a, e;
    if (moff) {
        a = (long long)up * moff[s];
        e = (long long)up * moff[s + 1];
    } else {
        a = (long long)s * L;
        e = a + L;
    }
    a = a < 0 ? 0 : (a > rows ? rows : a);
    e = e < a ? a : (e > rows ? rows : e);
    const long long nel = (e - a) * C;
    double sq = 0.0, ls = 0.0;
    const float* zs = z + a * ld_z;
    const bool dense = ld_z == C;             // no row stride: the segment is one contiguous run (no division per element)
    for (long long i = tid; i < nel; i += SW_THREADS) {
        const float v = dense ? zs[i] : zs[(i / C) * ld_z + i % C];
        sq += (double)v * (double)v;
    }
    for (long long r = a + tid; r < e; r += SW_THREADS) ls += (double)ls_row[r];
    s_sq[tid] = sq;
    s_ls[tid] = ls;
    __syncthreads();
    for (int w = SW_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_sq[tid] += s_sq[tid + w];
            s_ls[tid] += s_ls[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[2 * s] = s_sq[0];
        out[2 * s + 1] = s_ls[0];
    }
}

extern "C" int rtts_sw_nll_reduce(const float* z, int64_t ld_z, int C, const float* ls_row, const int32_t* moff, int nseg, int upsample,
                                  int64_t L, int64_t rows, double* out, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(z && ls_row && out && C > 0 && ld_z >= C && rows > 0 && upsample >= 1, "rtts_sw_nll_reduce: bad arguments");
    RTTS_REQUIRE(nseg >= 1 && nseg <= SW_MAX_SEGMENTS, "rtts_sw_nll_reduce: 1..%d segments (got %d)", SW_MAX_SEGMENTS, nseg);
    RTTS_REQUIRE(moff || (L > 0 && (int64_t)nseg * L == rows),
                 "rtts_sw_nll_reduce: without an offset table the rows are nseg segments of L rows (got nseg=%d, L=%lld, rows=%lld)", nseg,
                 (long long)L, (long long)rows);
    hipLaunchKernelGGL(sw_nll_reduce_kernel, dim3((unsigned)nseg), dim3(SW_THREADS), 0, (hipStream_t)stream, z, ld_z, C, ls_row, (const int*)moff,
                       upsample, (long long)L, (long long)rows, out);
    RTTS_LAUNCH_CHECK("rtts_sw_nll_reduce");
    return 0;
}

// Packed audio rows for the ragged likelihood, the audio twin of sw_pack_mel_kernel: dst (rows, C) fp32 contiguous, i.e.
// the reference's audio.unfold(1, C, C) (modules.py:304-306) of every utterance laid end to end.  Utterance s contributes
// exactly up * C * (moff[s+1] - moff[s]) samples (256 per mel frame for the reference's configurations), read from
// src[start[s] + j]; every element past the total, and any whose source index would fall outside [0, n_src), is zero.
__global__ __launch_bounds__(SW_THREADS) void sw_pack_audio_kernel(const float* __restrict__ src, long long n_src,
                                                                   const long long* __restrict__ start, const int* __restrict__ moff, int nseg,
                                                                   long long spf, size_t n, float* __restrict__ dst) {
    __shared__ int s_off[SW_MAX_SEGMENTS + 1];
    for (int i = threadIdx.x; i <= nseg; i += blockDim.x) s_off[i] = moff[i];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const long long f = (long long)(i / (size_t)spf);          // mel frame of this sample
        int lo = 0, hi = nseg + 1;                                 // s = (first offset above f) - 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= f) lo = mid + 1;
            else hi = mid;
        }
        const int s = lo - 1;
        float v = 0.f;
        if (s >= 0 && s < nseg && f < s_off[s + 1]) {
            const long long j = start[s] + ((long long)i - spf * s_off[s]);
            if (j >= 0 && j < n_src) v = src[j];
        }
        dst[i] = v;
    }
}

extern "C" int rtts_sw_pack_audio(const float* src, int64_t n_src, const int64_t* start, const int32_t* moff, int nseg, int upsample, int C,
                                  int64_t rows, float* dst, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(src && start && moff && dst && n_src > 0 && upsample >= 1 && C > 0 && rows > 0 && rows % upsample == 0,
                 "rtts_sw_pack_audio: bad arguments (rows a multiple of upsample)");
    RTTS_REQUIRE(nseg >= 1 && nseg <= SW_MAX_SEGMENTS, "rtts_sw_pack_audio: 1..%d segments (got %d)", SW_MAX_SEGMENTS, nseg);
    const size_t n = (size_t)rows * C;
    hipLaunchKernelGGL(sw_pack_audio_kernel, dim3(sw_grid(n)), dim3(SW_THREADS), 0, (hipStream_t)stream, src, (long long)n_src,
                       (const long long*)start, (const int*)moff, nseg, (long long)upsample * C, n, dst);
    RTTS_LAUNCH_CHECK("rtts_sw_pack_audio");
    return 0;
}
