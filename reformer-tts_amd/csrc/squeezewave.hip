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

// ================================================================== training: the backward of the analysis direction
// SqueezeWave.nll_backward differentiates SqueezeWaveLoss(SqueezeWave.forward) with the BatchNorms on batch statistics
// (reference reformer_tts/squeeze_wave/modules.py:100-117, :203-235, :294-332; loss.py:14-31).  The 1x1 convolutions'
// gradients are the MFMA GEMMs of gemm_nt.hip / gemm_tn.hip; the three pieces between them are here.  All of them are
// deterministic: no atomics, partial sums are added in a fixed order.

// ---- gate backward.  Forward (sw_gate_kernel): acts = t * g, t = tanh(p_t + c_t), g = sigmoid(p_s + c_s), the conditioning
// row r = (b, l / up) shared by `up` audio rows.  d_t = da * g * (1 - t^2), d_s = da * t * g * (1 - g); dpw[m] = [d_t | d_s]
// (bf16), and the conditioning row receives the fp32 sum over its `up` audio rows, rounded once.  One thread owns 8 channels of
// one CONDITIONING row and walks its audio rows in order, so the sum needs no second pass.
__global__ __launch_bounds__(SW_THREADS) void sw_gate_bwd_kernel(const bf16_t* __restrict__ pw, const bf16_t* __restrict__ cond, int64_t ld_cond,
                                                                 int off, int up, int C, size_t n8, const bf16_t* __restrict__ dacts,
                                                                 bf16_t* __restrict__ dpw, bf16_t* __restrict__ dcond, int64_t ld_dcond) {
    const int c8 = C / 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c8) * 8;
        const size_t crow = i / c8;               // (b, lm): its audio rows are crow * up + j (L = Lm * up)
        const uint4 ct = *reinterpret_cast<const uint4*>(cond + crow * ld_cond + off + c);
        const uint4 cs = *reinterpret_cast<const uint4*>(cond + crow * ld_cond + off + C + c);
        const uint32_t e[4] = {ct.x, ct.y, ct.z, ct.w}, f[4] = {cs.x, cs.y, cs.z, cs.w};
        float st[8], ss[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) st[j] = ss[j] = 0.f;
        for (int u = 0; u < up; ++u) {
            const size_t row = crow * up + u;
            const uint4 pt = *reinterpret_cast<const uint4*>(pw + row * 2 * C + c);
            const uint4 ps = *reinterpret_cast<const uint4*>(pw + row * 2 * C + C + c);
            const uint4 da = *reinterpret_cast<const uint4*>(dacts + row * C + c);
            const uint32_t a[4] = {pt.x, pt.y, pt.z, pt.w}, bq[4] = {ps.x, ps.y, ps.z, ps.w}, d[4] = {da.x, da.y, da.z, da.w};
            uint32_t ot[4], os[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float dt[2], ds[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float tin = h ? __uint_as_float(a[j] & 0xffff0000u) + __uint_as_float(e[j] & 0xffff0000u)
                                        : __uint_as_float(a[j] << 16) + __uint_as_float(e[j] << 16);
                    const float sin_ = h ? __uint_as_float(bq[j] & 0xffff0000u) + __uint_as_float(f[j] & 0xffff0000u)
                                         : __uint_as_float(bq[j] << 16) + __uint_as_float(f[j] << 16);
                    const float g = h ? __uint_as_float(d[j] & 0xffff0000u) : __uint_as_float(d[j] << 16);
                    const float t = tanhf(tin), sg = 1.f / (1.f + __expf(-sin_));
                    dt[h] = g * sg * (1.f - t * t);
                    ds[h] = g * t * sg * (1.f - sg);
                    st[2 * j + h] += dt[h];
                    ss[2 * j + h] += ds[h];
                }
                ot[j] = pack_bf16x2(dt[0], dt[1]);
                os[j] = pack_bf16x2(ds[0], ds[1]);
            }
            *reinterpret_cast<uint4*>(dpw + row * 2 * C + c) = make_uint4(ot[0], ot[1], ot[2], ot[3]);
            *reinterpret_cast<uint4*>(dpw + row * 2 * C + C + c) = make_uint4(os[0], os[1], os[2], os[3]);
        }
        *reinterpret_cast<uint4*>(dcond + crow * ld_dcond + off + c) =
            make_uint4(pack_bf16x2(st[0], st[1]), pack_bf16x2(st[2], st[3]), pack_bf16x2(st[4], st[5]), pack_bf16x2(st[6], st[7]));
        *reinterpret_cast<uint4*>(dcond + crow * ld_dcond + off + C + c) =
            make_uint4(pack_bf16x2(ss[0], ss[1]), pack_bf16x2(ss[2], ss[3]), pack_bf16x2(ss[4], ss[5]), pack_bf16x2(ss[6], ss[7]));
    }
}

extern "C" int rtts_sw_gate_bwd(const void* pw, const void* cond, int64_t ld_cond, int cond_offset, int upsample, int B, int L, int Lm, int C,
                                const void* dacts, void* dpw, void* dcond, int64_t ld_dcond, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(pw && cond && dacts && dpw && dcond && B > 0 && L > 0 && Lm > 0 && C > 0 && C % 8 == 0 && cond_offset >= 0 &&
                     cond_offset % 8 == 0 && ld_cond % 8 == 0 && ld_dcond % 8 == 0 && upsample >= 1 && (int64_t)Lm * upsample == L &&
                     ld_cond >= cond_offset + 2 * C && ld_dcond >= cond_offset + 2 * C,
                 "rtts_sw_gate_bwd: bad arguments (C %% 8 == 0, L == Lm * upsample, leading dimensions >= cond_offset + 2 C)");
    RTTS_REQUIRE(dpw != pw && dcond != cond, "rtts_sw_gate_bwd: not in place");
    RTTS_REQUIRE((((uintptr_t)pw | (uintptr_t)cond | (uintptr_t)dacts | (uintptr_t)dpw | (uintptr_t)dcond) & 15) == 0,
                 "rtts_sw_gate_bwd: pw, cond, dacts, dpw and dcond must be 16-byte aligned (8 bf16 channels per access)");
    const size_t n8 = (size_t)B * Lm * C / 8;
    hipLaunchKernelGGL(sw_gate_bwd_kernel, dim3(sw_grid(n8)), dim3(SW_THREADS), 0, (hipStream_t)stream, (const bf16_t*)pw, (const bf16_t*)cond,
                       ld_cond, cond_offset, upsample, C, n8, (const bf16_t*)dacts, (bf16_t*)dpw, (bf16_t*)dcond, ld_dcond);
    RTTS_LAUNCH_CHECK("rtts_sw_gate_bwd");
    return 0;
}

// ---- depthwise k3 + batch-statistics BatchNorm backward, two passes.  Forward: xhat = (h - mean) * rstd, u = gamma * xhat +
// beta, y_l = b + sum_k w_k u_{l+k-1} with u zero outside the utterance.  Given dy (bf16):
//     du_l = w_0 dy_{l+1} + w_1 dy_l + w_2 dy_{l-1}   (dy zero outside the utterance)
//     sums[0..3) = d w_k = sum dy_l u_{l+k-1},  sums[3] = d b = sum dy,  sums[4] = d gamma = sum du xhat,  sums[5] = d beta = sum du
//     dh += gamma rstd (du - sums[5] / m - xhat sums[4] / m),   m = B * L
// Pass 1: a workgroup owns a slab of rows; a thread owns 8 channels and every R-th row of the slab, R = 256 / min(C/8, 64); the
// R row lanes are added in order through LDS and the slab's six sums go to partial[slab][6][C]; a second launch adds the slabs
// in order.  Pass 2 is elementwise.
#define SWB_SUMS 6
#define SWB_MAX_SLABS 256

struct SwbRow {
    float dy[8], du[8], u[3][8], xh[8];
};

__device__ __forceinline__ void swb_load8(const float* __restrict__ p, float* o) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// everything pass 1 and 2 need of row `row` for the 8 channels from c on: 16-byte accesses (8 bf16 of dy, 2 x 4 fp32 of h)
__device__ __forceinline__ void swb_load(const float* __restrict__ h, const bf16_t* __restrict__ dy, size_t row, int l, int L, int C, int c,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta, const float* w,
                                         bool want_u, SwbRow& r) {
    const bool first = l == 0, last = l + 1 == L;
    uint4 dlo = make_uint4(0u, 0u, 0u, 0u), dhi = dlo;
    if (!first) dlo = *reinterpret_cast<const uint4*>(dy + (row - 1) * C + c);
    if (!last) dhi = *reinterpret_cast<const uint4*>(dy + (row + 1) * C + c);
    float d0[8], dl[8], dh[8], hm[8], hl[8], hh[8];
    rtts_unpack8(*reinterpret_cast<const uint4*>(dy + row * C + c), d0);
    rtts_unpack8(dlo, dl);
    rtts_unpack8(dhi, dh);
    swb_load8(h + row * C + c, hm);
#pragma unroll
    for (int j = 0; j < 8; ++j) hl[j] = hh[j] = 0.f;
    if (want_u) {
        if (!first) swb_load8(h + (row - 1) * C + c, hl);
        if (!last) swb_load8(h + (row + 1) * C + c, hh);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* wc = w + (size_t)(c + j) * 3;
        r.dy[j] = d0[j];
        r.du[j] = __builtin_fmaf(wc[0], dh[j], __builtin_fmaf(wc[1], d0[j], wc[2] * dl[j]));
        const float mu = mean[c + j], rs = rstd[c + j], ga = gamma[c + j], be = beta[c + j];
        r.xh[j] = (hm[j] - mu) * rs;
        if (want_u) {
            r.u[1][j] = __builtin_fmaf(ga, r.xh[j], be);
            r.u[0][j] = first ? 0.f : __builtin_fmaf(ga, (hl[j] - mu) * rs, be);
            r.u[2][j] = last ? 0.f : __builtin_fmaf(ga, (hh[j] - mu) * rs, be);
        }
    }
}

__global__ __launch_bounds__(SW_THREADS) void sw_dwbn_bwd_partial_kernel(const float* __restrict__ h, const bf16_t* __restrict__ dy,
                                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                         const float* __restrict__ w, int L, int C, long long rows,
                                                                         int slab_rows, float* __restrict__ partial) {
    __shared__ float red[SW_THREADS][8 * SWB_SUMS + 1];
    const int c8 = C / 8, cq = c8 < 64 ? c8 : 64, R = SW_THREADS / cq;
    const int tid = threadIdx.x, lane_c = tid % cq, lane_r = tid / cq;
    const int q = blockIdx.y * 64 + lane_c;                     // group of 8 channels
    const bool live = lane_r < R && q < c8;
    float acc[SWB_SUMS][8];
#pragma unroll
    for (int s = 0; s < SWB_SUMS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[s][j] = 0.f;
    if (live) {
        const long long r0 = (long long)blockIdx.x * slab_rows;
        long long r1 = r0 + slab_rows;
        if (r1 > rows) r1 = rows;
        for (long long row = r0 + lane_r; row < r1; row += R) {
            SwbRow r;
            swb_load(h, dy, (size_t)row, (int)(row % L), L, C, q * 8, mean, rstd, gamma, beta, w, true, r);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc[0][j] = __builtin_fmaf(r.dy[j], r.u[0][j], acc[0][j]);
                acc[1][j] = __builtin_fmaf(r.dy[j], r.u[1][j], acc[1][j]);
                acc[2][j] = __builtin_fmaf(r.dy[j], r.u[2][j], acc[2][j]);
                acc[3][j] += r.dy[j];
                acc[4][j] = __builtin_fmaf(r.du[j], r.xh[j], acc[4][j]);
                acc[5][j] += r.du[j];
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SWB_SUMS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) red[tid][s * 8 + j] = acc[s][j];
    __syncthreads();
    if (live && lane_r == 0) {
#pragma unroll
        for (int s = 0; s < SWB_SUMS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = red[lane_c][s * 8 + j];
                for (int rr = 1; rr < R; ++rr) t += red[rr * cq + lane_c][s * 8 + j];
                partial[((size_t)blockIdx.x * SWB_SUMS + s) * C + q * 8 + j] = t;
            }
    }
}

__global__ __launch_bounds__(SW_THREADS) void sw_dwbn_bwd_final_kernel(const float* __restrict__ partial, int nslabs, int C, float* __restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;       // (sum, channel)
    if (i >= SWB_SUMS * C) return;
    float t = 0.f;
    for (int s = 0; s < nslabs; ++s) t += partial[(size_t)s * SWB_SUMS * C + i];
    sums[i] = t;
}

__global__ __launch_bounds__(SW_THREADS) void sw_dwbn_bwd_apply_kernel(const float* __restrict__ h, const bf16_t* __restrict__ dy,
                                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                       const float* __restrict__ w, const float* __restrict__ sums, int L, int C,
                                                                       size_t n8, float inv_m, float* __restrict__ dh) {
    const int c8 = C / 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c8) * 8;
        const size_t row = i / c8;
        SwbRow r;
        swb_load(h, dy, row, (int)(row % L), L, C, c, mean, rstd, gamma, beta, w, false, r);
        float op[8];
        swb_load8(dh + row * C + c, op);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = gamma[c + j] * rstd[c + j];
            op[j] += a * (r.du[j] - sums[5 * C + c + j] * inv_m - r.xh[j] * (sums[4 * C + c + j] * inv_m));
        }
        *reinterpret_cast<float4*>(dh + row * C + c) = make_float4(op[0], op[1], op[2], op[3]);
        *reinterpret_cast<float4*>(dh + row * C + c + 4) = make_float4(op[4], op[5], op[6], op[7]);
    }
}

static int swb_slab_rows(long long rows) {
    long long s = (rows + SWB_MAX_SLABS - 1) / SWB_MAX_SLABS;
    if (s < 16) s = 16;
    return (int)s;
}

extern "C" int rtts_sw_dwbn_bwd_partial_floats(int64_t rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    const int sr = swb_slab_rows(rows);
    return (int)((rows + sr - 1) / sr) * SWB_SUMS * C;
}

extern "C" int rtts_sw_dwbn_bwd_sums(const float* h, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     const float* w, int B, int L, int C, float* sums, float* partial_ws, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(h && dy && mean && rstd && gamma && beta && w && sums && partial_ws && B > 0 && L > 0 && C > 0 && C % 8 == 0 &&
                     (int64_t)B * L < (1ll << 31) / 4,
                 "rtts_sw_dwbn_bwd_sums: bad arguments (C %% 8 == 0)");
    RTTS_REQUIRE((((uintptr_t)h | (uintptr_t)dy) & 15) == 0, "rtts_sw_dwbn_bwd_sums: h and dy must be 16-byte aligned (8 channels per access)");
    const long long rows = (long long)B * L;
    const int sr = swb_slab_rows(rows), nslabs = (int)((rows + sr - 1) / sr);
    hipLaunchKernelGGL(sw_dwbn_bwd_partial_kernel, dim3(nslabs, (C / 8 + 63) / 64), dim3(SW_THREADS), 0, (hipStream_t)stream, h, (const bf16_t*)dy,
                       mean, rstd, gamma, beta, w, L, C, rows, sr, partial_ws);
    hipLaunchKernelGGL(sw_dwbn_bwd_final_kernel, dim3((SWB_SUMS * C + SW_THREADS - 1) / SW_THREADS), dim3(SW_THREADS), 0, (hipStream_t)stream,
                       partial_ws, nslabs, C, sums);
    RTTS_LAUNCH_CHECK("rtts_sw_dwbn_bwd_sums");
    return 0;
}

extern "C" int rtts_sw_dwbn_bwd_apply(const float* h, const void* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                      const float* w, const float* sums, int B, int L, int C, float* dh, void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(h && dy && mean && rstd && gamma && beta && w && sums && dh && B > 0 && L > 0 && C > 0 && C % 8 == 0,
                 "rtts_sw_dwbn_bwd_apply: bad arguments (C %% 8 == 0)");
    RTTS_REQUIRE(dh != h, "rtts_sw_dwbn_bwd_apply: dh must not alias h");
    RTTS_REQUIRE((((uintptr_t)h | (uintptr_t)dh | (uintptr_t)dy) & 15) == 0,
                 "rtts_sw_dwbn_bwd_apply: h, dh and dy must be 16-byte aligned (8 channels per access)");
    const size_t n8 = (size_t)B * L * C / 8;
    hipLaunchKernelGGL(sw_dwbn_bwd_apply_kernel, dim3(sw_grid(n8)), dim3(SW_THREADS), 0, (hipStream_t)stream, h, (const bf16_t*)dy, mean, rstd, gamma,
                       beta, w, sums, L, C, n8, 1.f / (float)((size_t)B * L), dh);
    RTTS_LAUNCH_CHECK("rtts_sw_dwbn_bwd_apply");
    return 0;
}

// ---- flow-boundary backward, the mirror of sw_coupling_fwd1x1_kernel.  That launch computed, from the previous flow's conv
// output x = [x0 | x1] and WN output wn = [log_s | b]:  c = [x0 | exp(log_s) x1 + b],  z[:, z_col : +n_early] = c[:, :n_early],
// out = c[:, n_early:] W^T.  Given dout (rows, n) and the loss's z-seed dz = z * z_scale (z_scale = 1 / (sigma^2 N)):
//     dc = [z[:, z_col : +n_early] * z_scale | dout W]
//     dW_part[block] = sum over the block's rows of dout^T c[:, n_early:]       (c recomputed as the forward computed it)
//     dx = [dc_0 | dc_1 exp(log_s)],   dwn = [dc_1 x1 exp(log_s) - inv_n | dc_1]   (inv_n = 1 / N: the loss's -sum log_s / N)
// wn NULL (the first flow): x is the audio, which needs no gradient -- only dW is produced.  w NULL (the tail): n = 0,
// dc = dz.  A workgroup walks the 32-row tiles blockIdx.x, blockIdx.x + gridDim.x, ... in order with its share of dW (thread
// (ti, tk) owns elements (ti + 16 a, tk + 16 b)) in registers; a second launch adds the workgroups' shares in order.
#define SWD_MAX_BLOCKS 256
__global__ __launch_bounds__(SW_THREADS) void sw_boundary_bwd_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ wn,
                                                                     int64_t ld_wn, const float* __restrict__ w, int n_in, int n_early,
                                                                     long long rows, const float* __restrict__ dout, int64_t ld_dout,
                                                                     const float* __restrict__ z, int64_t ld_z, int z_col, float z_scale,
                                                                     float inv_n, float* __restrict__ dx, int64_t ld_dx,
                                                                     float* __restrict__ dwn, int64_t ld_dwn, float* __restrict__ dw_part) {
    extern __shared__ __attribute__((aligned(16))) float swd_smem[];
    const int n = n_in - n_early, half = n_in / 2;
    float* W = swd_smem;                      // [n][n] row-major, as given
    float* DX = W + n * n;                    // [SWI_ROWS][n + 1]: dout
    float* CC = DX + SWI_ROWS * (n + 1);      // [SWI_ROWS][n_in + 1]: the coupled rows
    const int tid = threadIdx.x;
    if (w)
        for (int i = tid; i < n * n; i += SW_THREADS) W[i] = w[i];
    const int ti = tid >> 4, tk = tid & 15;
    float acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.f;
    const long long tiles = (rows + SWI_ROWS - 1) / SWI_ROWS;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r0 = tile * SWI_ROWS;
        __syncthreads();                      // the previous tile's readers are done (and W is in place)
        for (int i = tid; i < SWI_ROWS * n; i += SW_THREADS) {
            const int rr = i / n, k = i % n;
            const long long row = r0 + rr;
            DX[rr * (n + 1) + k] = row < rows ? dout[row * ld_dout + k] : 0.f;
        }
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
            CC[rr * (n_in + 1) + k] = v;
        }
        __syncthreads();
        if (w) {
            for (int rr = 0; rr < SWI_ROWS; ++rr) {
                const float* dr = DX + rr * (n + 1);
                const float* cr = CC + rr * (n_in + 1) + n_early;
                float dv[8], cv[8];
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    dv[a] = ti + 16 * a < n ? dr[ti + 16 * a] : 0.f;
                    cv[a] = tk + 16 * a < n ? cr[tk + 16 * a] : 0.f;
                }
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) acc[a][b] = __builtin_fmaf(dv[a], cv[b], acc[a][b]);
            }
        }
        if (!wn) continue;                    // the first flow: no coupling in front of it, the audio needs no gradient
        const int rr = tid >> 3, g = tid & 7;
        const long long row = r0 + rr;
        if (row >= rows) continue;
        const float* dr = DX + rr * (n + 1);
        for (int k = g; k < n_in; k += 8) {
            float dc;
            if (k < n_early) {
                dc = z[row * ld_z + z_col + k] * z_scale;
            } else {
                dc = 0.f;
                const float* wk = W + (k - n_early);
                for (int i = 0; i < n; ++i) dc = __builtin_fmaf(dr[i], wk[(size_t)i * n], dc);
            }
            if (k < half) {
                dx[row * ld_dx + k] = dc;
            } else {
                const float es = __expf(wn[row * ld_wn + (k - half)]), x1 = x[row * ld_x + k];
                dx[row * ld_dx + k] = dc * es;
                dwn[row * ld_dwn + (k - half)] = __builtin_fmaf(dc * x1, es, -inv_n);
                dwn[row * ld_dwn + k] = dc;
            }
        }
    }
    if (!w) return;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b)
            if (ti + 16 * a < n && tk + 16 * b < n) dw_part[(size_t)blockIdx.x * n * n + (size_t)(ti + 16 * a) * n + tk + 16 * b] = acc[a][b];
}

__global__ __launch_bounds__(SW_THREADS) void sw_boundary_bwd_final_kernel(const float* __restrict__ part, int nblocks, int nn, float* __restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nn) return;
    float t = 0.f;
    for (int p = 0; p < nblocks; ++p) t += part[(size_t)p * nn + i];
    dw[i] = t;
}

static RttsLdsState g_swd_lds;

extern "C" int rtts_sw_boundary_bwd_blocks(int64_t rows) {
    if (rows <= 0) return 0;
    const int64_t tiles = (rows + SWI_ROWS - 1) / SWI_ROWS;
    return (int)(tiles < SWD_MAX_BLOCKS ? tiles : SWD_MAX_BLOCKS);
}

extern "C" int rtts_sw_boundary_bwd(const float* x, int64_t ld_x, const float* wn_out, int64_t ld_wn, const float* w, int n_in, int n_early,
                                    int64_t rows, const float* dout, int64_t ld_dout, const float* z, int64_t ld_z, int z_col, float z_scale,
                                    float inv_n, float* dx, int64_t ld_dx, float* dwn, int64_t ld_dwn, float* dw, float* partial_ws,
                                    void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(n_in >= 2 && n_in % 2 == 0 && n_in <= SWI_MAXN, "rtts_sw_boundary_bwd: n_in must be even and <= %d (got n_in=%d)", SWI_MAXN, n_in);
    RTTS_REQUIRE(n_early >= 0 && n_early <= n_in && n_early % 2 == 0,
                 "rtts_sw_boundary_bwd: n_early must be even and within [0, n_in] (got n_early=%d, n_in=%d)", n_early, n_in);
    const int n = n_in - n_early;
    RTTS_REQUIRE(x && rows > 0 && ld_x >= n_in, "rtts_sw_boundary_bwd: bad arguments (x, rows > 0, ld_x >= n_in)");
    RTTS_REQUIRE(wn_out || w, "rtts_sw_boundary_bwd: nothing to do without wn_out and w");
    if (wn_out) {
        RTTS_REQUIRE(ld_wn >= n_in && dx && dwn && ld_dx >= n_in && ld_dwn >= n_in,
                     "rtts_sw_boundary_bwd: the coupling needs dx and dwn with leading dimensions >= n_in");
        RTTS_REQUIRE(dx != x && dx != dout && dwn != wn_out && (const float*)dx != z, "rtts_sw_boundary_bwd: not in place");
        RTTS_REQUIRE(n_early == 0 || (z && z_col >= 0 && ld_z >= (int64_t)z_col + n_early),
                     "rtts_sw_boundary_bwd: the early output's gradient needs z with ld_z >= z_col + n_early (got z_col=%d, n_early=%d)", z_col,
                     n_early);
    }
    if (w) {
        RTTS_REQUIRE(n >= 2 && dout && ld_dout >= n && dw && partial_ws,
                     "rtts_sw_boundary_bwd: the convolution needs n = n_in - n_early >= 2, dout with ld_dout >= n, dw and partial_ws");
    } else {
        RTTS_REQUIRE(n == 0, "rtts_sw_boundary_bwd: without W every column is early output: n_early must equal n_in (got %d, %d)", n_early, n_in);
    }
    const size_t lds = ((size_t)n * n + (size_t)SWI_ROWS * (n + 1) + (size_t)SWI_ROWS * (n_in + 1)) * sizeof(float);
    RTTS_ENSURE_LDS("rtts_sw_boundary_bwd", sw_boundary_bwd_kernel, lds, g_swd_lds);
    const int blocks = rtts_sw_boundary_bwd_blocks(rows);
    hipLaunchKernelGGL(sw_boundary_bwd_kernel, dim3(blocks), dim3(SW_THREADS), lds, (hipStream_t)stream, x, ld_x, wn_out, ld_wn, w, n_in, n_early,
                       (long long)rows, dout, ld_dout, z, ld_z, z_col, z_scale, inv_n, dx, ld_dx, dwn, ld_dwn, partial_ws);
    if (w)
        hipLaunchKernelGGL(sw_boundary_bwd_final_kernel, dim3((n * n + SW_THREADS - 1) / SW_THREADS), dim3(SW_THREADS), 0, (hipStream_t)stream,
                           partial_ws, blocks, n * n, dw);
    RTTS_LAUNCH_CHECK("rtts_sw_boundary_bwd");
    return 0;
}
