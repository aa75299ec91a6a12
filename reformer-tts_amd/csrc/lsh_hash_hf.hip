// LSH bucket assignment + stable counting sort of the HuggingFace layer (implementation="huggingface_transformers").
//
// Replaces LSHSelfAttention._hash_vectors / _get_sorted_bucket_idx_and_undo_sorted_bucket_idx of transformers'
// models/reformer/modeling_reformer.py, which the reference binds at reformer_tts/model/reformer.py:201-220.  What differs from
// lsh_hash_sort.hip (the reformer_pytorch branch):
//   * the bucket count is an argument (2 .. 256, even), not T / bucket_size;
//   * rotations are per HEAD and shared over the batch: (H, dh, n_hashes, n_buckets / 2), row = bh % H;
//   * with a mask, masked tokens take the extra bucket n_buckets and round r is offset by r * (n_buckets + 1).
// Same structure as the two-launch form there:
//   * hash kernel: a workgroup = 128 tokens of one (batch, head), 32 per wave; the rows are fetched and staged ONCE and
//     projected on the columns of every round by v_mfma_f32_32x32x2_f32 -- bit for bit the k-ordered fp32 fmaf chain of
//     oracle/lsh_int.c (one rounding per product, no wider accumulation).  The A operand is R^T with the rounds side by side, 32
//     columns per pass; from 64 columns per round on a round takes several passes and the first maximum over [xR, -xR] is
//     carried across them.  Bucket ids go to `st` (as scratch) and to `buckets`.
//   * sort kernel: one workgroup per (head, round) runs the ballot-based stable counting sort over up to 257 bins.
// LDS layout of the histogram: one row of counters per wave, 64 * SEG words long with SEG odd.  The adds and the per-bucket
// sums touch consecutive words (conflict-free whatever the row length); the exclusive scan gives lane l the SEG consecutive
// words l * SEG ..: ds_read_b32 banks are (address / 4) % 32 per 32-lane half, so an odd SEG puts the 32 lanes of a half on 32
// different banks, where the even lengths that 128 or 256 bins suggest (2, 4) would make every read 2- or 4-way.
#include "rtts_common.h"
#include "attn_tile.h"   // AT_PADB

#define HH_DH 64
#define HH_W8_MIN_T 2048

// HALFC = the compile-time column capacity of a round (a power of two >= half, 1 .. 128), half = n_buckets / 2 of this call.
// A pass is 32 columns of the (round, column) grid: 32 / HALFC rounds side by side while a round fits (the decoder of
// config/huggingface-lsh.yml: 16 buckets, 8 rounds x 8 columns = TWO passes), HALFC / 32 passes per round above that.
template <int HALFC>
__global__ __launch_bounds__(256) void lsh_hash_hf_kernel(const bf16_t* __restrict__ qk, int64_t ld, const float* __restrict__ rotations,
                                                          const uint8_t* __restrict__ mask, int H, int T, int n_hashes, int half,
                                                          int stride, int32_t* __restrict__ buckets, int32_t* __restrict__ ids) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[4 * 32 * AT_PADB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blocks_per_head = T / 128;
    const uint32_t w = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = w / blocks_per_head, t0 = (w % blocks_per_head) * 128 + wave * 32;
    const int b = bh / H, h = bh % H;
    const bf16_t* base = qk + ((size_t)b * T + t0) * ld + (size_t)h * HH_DH;
    unsigned char* wt = tile + wave * 32 * AT_PADB;
    {   // stage this wave's 32 rows: coalesced 16-byte pieces, all four loads in flight
        uint4 pre[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) pre[p] = *reinterpret_cast<const uint4*>(base + (size_t)(p * 8 + (lane >> 3)) * ld + (lane & 7) * 8);
#pragma unroll
        for (int p = 0; p < 4; ++p) *reinterpret_cast<uint4*>(wt + (p * 8 + (lane >> 3)) * AT_PADB + (lane & 7) * 16) = pre[p];
    }
    __builtin_amdgcn_wave_barrier();      // same wave wrote and reads: LDS ops of one wave execute in order
    const int hh = lane >> 5, l31 = lane & 31;
    // B operand: q[token][2j + hh], token = lane & 31: 32 registers, kept for every pass
    float bq[32];
    {
        const unsigned char* rowp = wt + l31 * AT_PADB;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const uint4 val = *reinterpret_cast<const uint4*>(rowp + p * 16);
            const uint32_t uu[4] = {val.x, val.y, val.z, val.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) bq[p * 4 + k] = __uint_as_float(hh ? (uu[k] & 0xffff0000u) : (uu[k] << 16));
        }
    }
    const int tok = t0 + l31;
    const bool valid = mask ? mask[(size_t)b * T + tok] != 0 : true;
    const int pad = 2 * half;                                                     // the padding bucket of masked tokens
    const float* rot_src = rotations + (size_t)h * HH_DH * n_hashes * half;       // per head, shared over the batch
    int32_t* ids_h = ids + (size_t)bh * n_hashes * T + tok;
    int32_t* buckets_h = buckets ? buckets + (size_t)bh * n_hashes * T + tok : nullptr;
    constexpr int CW = HALFC < 32 ? HALFC : 32;       // columns of one round inside a pass
    constexpr int RPP = 32 / CW;                      // rounds per pass
    constexpr int PPR = HALFC / CW;                   // passes per round
    for (int r0 = 0; r0 < n_hashes; r0 += RPP) {
        // first maximum of +x and of -x over this lane's columns of each round, ascending column (CW >= 8 only)
        float bp[RPP], bn[RPP];
        int ip[RPP], in[RPP];
#pragma unroll
        for (int q = 0; q < RPP; ++q) { bp[q] = bn[q] = -__builtin_inff(); ip[q] = in[q] = 0; }
#pragma unroll
        for (int pp = 0; pp < PPR; ++pp) {
            // A operand: column lane & 31 of this pass = (round r0 + l31 / CW, column 32 pp + l31 % CW), rows 2j + hh; zero outside
            // the real grid
            const int ar = r0 + l31 / CW, aci = 32 * pp + l31 % CW;
            const bool areal = ar < n_hashes && aci < half;
            float rot_reg[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) rot_reg[j] = areal ? rot_src[((size_t)(2 * j + hh) * n_hashes + ar) * half + aci] : 0.f;
            f32x16 acc = {0};
#pragma unroll
            for (int j = 0; j < 32; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rot_reg[j], bq[j], acc, 0, 0, 0);
            // acc[i] = projection of token lane & 31 on column m = 8 (i >> 2) + 4 hh + (i & 3) of the pass; argmax over [xR, -xR]
            // of each round, the first maximum winning (ascending column, +x before -x)
            if constexpr (CW <= 4) {
                // a lane's group g (four consecutive columns) holds 4 / CW complete rounds: no other lane has a share in them
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int jr = 0; jr < 4 / CW; ++jr) {
                        const int rr = r0 + (8 * g + 4 * hh) / CW + jr;
                        float best = -__builtin_inff();
                        int bi = 0;
#pragma unroll
                        for (int ci = 0; ci < CW; ++ci) {
                            const float x = acc[4 * g + jr * CW + ci];
                            if (ci < half && x > best) { best = x; bi = ci; }
                        }
#pragma unroll
                        for (int ci = 0; ci < CW; ++ci) {
                            const float x = -acc[4 * g + jr * CW + ci];
                            if (ci < half && x > best) { best = x; bi = half + ci; }
                        }
                        if (!valid) bi = pad;
                        if (rr < n_hashes) {
                            ids_h[(size_t)rr * T] = bi;
                            if (buckets_h) buckets_h[(size_t)rr * T] = bi + rr * stride;
                        }
                    }
            } else {
                // a round spans both lane halves and CW / 8 groups (and, from 64 columns on, several passes)
                constexpr int GPR = CW / 8;
#pragma unroll
                for (int q = 0; q < RPP; ++q)
#pragma unroll
                    for (int gg = 0; gg < GPR; ++gg)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int ci = 32 * pp + 8 * gg + 4 * hh + j;
                            const float x = acc[4 * (q * GPR + gg) + j];
                            if (ci < half && x > bp[q]) { bp[q] = x; ip[q] = ci; }
                            if (ci < half && -x > bn[q]) { bn[q] = -x; in[q] = ci; }
                        }
            }
        }
        if constexpr (CW >= 8) {
#pragma unroll
            for (int q = 0; q < RPP; ++q) {
                // [xR, -xR]: every +column precedes every -column, so +x keeps a tie
                float best = bp[q];
                int bi = ip[q];
                if (bn[q] > bp[q]) { best = bn[q]; bi = half + in[q]; }
                // the partner half holds the other columns of the same token: larger value wins, the smaller index on a tie
                const auto sv = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);
                const auto si = __builtin_amdgcn_permlane32_swap((unsigned)bi, (unsigned)bi, false, false);
                const float ob = __uint_as_float(hh ? sv[0] : sv[1]);
                const int oi = (int)(hh ? si[0] : si[1]);
                int idx = (ob > best || (ob == best && oi < bi)) ? oi : bi;
                if (!valid) idx = pad;
                const int rr = r0 + q;
                if (rr < n_hashes && hh == (rr & 1)) {       // both halves know the result: they take turns storing
                    ids_h[(size_t)rr * T] = idx;
                    if (buckets_h) buckets_h[(size_t)rr * T] = idx + rr * stride;
                }
            }
        }
    }
}

// lanes of the wave whose value v (0 <= v < 2^BITS, or -1 = inactive) equals this lane's
template <int BITS>
__device__ __forceinline__ unsigned long long hf_match_lanes(int v) {
    unsigned long long m = __ballot(v >= 0);
#pragma unroll
    for (int bit = 0; bit < BITS; ++bit) {
        const unsigned long long bm = __ballot((v >> bit) & 1);
        m &= ((v >> bit) & 1) ? bm : ~bm;
    }
    return m;
}

// histogram step of one wave (see count_lanes of lsh_hash_sort.hip): with few bins the first lane of each group of equal values
// adds the group's size (no same-address serialisation), with many bins equal values are rare and the plain LDS add is cheaper
template <int BITS>
__device__ __forceinline__ void hf_count_lanes(int* cnt, int v, int lane) {
    if constexpr (BITS <= 4) {
        const unsigned long long m = hf_match_lanes<BITS>(v);
        if (v >= 0 && (m & ((1ull << lane) - 1ull)) == 0) cnt[v] += __popcll(m);
    } else {
        if (v >= 0) atomicAdd(&cnt[v], 1);                     // integer LDS add: order-free, deterministic
    }
}

// stable counting sort of one (head, round): ids (in `st`, written by the hash kernel) -> st (sorted slot -> token), undo.
// NB bins (<= 64 * SEG, SEG odd), 2^BITS >= NB.
template <int BITS, int SEG, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void lsh_sort_ids_hf_kernel(int T, int NB, int32_t* __restrict__ st, int32_t* __restrict__ undo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ROW = 64 * SEG;              // words per counter row
    constexpr int NTHR = 64 * WAVES;
    uint16_t* bkt = reinterpret_cast<uint16_t*>(smem);
    int* cntw = reinterpret_cast<int*>(smem + ((T * 2 + 15) & ~15));      // [WAVES][ROW]
    int* tot = cntw + WAVES * ROW;                                        // [ROW]: per-bin totals, then their exclusive prefix
    const uint32_t w = xcd_remap(blockIdx.x, gridDim.x);                  // (head, round) in the order of the arrays
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* st_out = st + (size_t)w * T;
    int32_t* undo_out = undo ? undo + (size_t)w * T : nullptr;
    const int seg = T / WAVES, s0 = wave * seg;
    for (int i = tid; i < (WAVES + 1) * ROW; i += NTHR) cntw[i] = 0;       // the totals' row too: the scan reads all of it
    __syncthreads();
    for (int t0 = 0; t0 < seg; t0 += 64) {                     // wave w counts the segment it will place
        const bool act = t0 + lane < seg;
        int id = act ? st_out[s0 + t0 + lane] : -1;
        if (id >= NB) id = NB - 1;                             // cannot happen (the hash kernel writes < NB): keeps the LDS adds in bounds
        if (act) bkt[s0 + t0 + lane] = (uint16_t)id;
        hf_count_lanes<BITS>(cntw + wave * ROW, id, lane);     // this wave's own row of counters
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();                                           // all ids are in LDS: st may be overwritten from here on
    for (int k = tid; k < NB; k += NTHR) {
        int t = 0;
#pragma unroll
        for (int w2 = 0; w2 < WAVES; ++w2) t += cntw[w2 * ROW + k];
        tot[k] = t;
    }
    __syncthreads();
    if (wave == 0) {
        // exclusive prefix over the ROW totals: lane l owns words l * SEG .. l * SEG + SEG - 1 (SEG odd: conflict-free)
        int v[SEG], sum = 0;
#pragma unroll
        for (int j = 0; j < SEG; ++j) { v[j] = tot[lane * SEG + j]; sum += v[j]; }
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        int run0 = incl - sum;
#pragma unroll
        for (int j = 0; j < SEG; ++j) { tot[lane * SEG + j] = run0; run0 += v[j]; }
    }
    __syncthreads();
    // first sorted slot of (bin k, wave w) = tokens in smaller bins + tokens of bin k in earlier waves' segments
    int basek[SEG];
#pragma unroll
    for (int j = 0; j < SEG; ++j) {
        const int k = lane + 64 * j;
        int bk = 0;
        if (k < NB) {
            bk = tot[k];
            for (int w2 = 0; w2 < wave; ++w2) bk += cntw[w2 * ROW + k];
        }
        basek[j] = bk;
    }
    __syncthreads();                         // every wave has read the counts before they become running offsets
    int* run = cntw + wave * ROW;            // this wave's running offset per bin
#pragma unroll
    for (int j = 0; j < SEG; ++j)
        if (lane + 64 * j < NB) run[lane + 64 * j] = basek[j];
    __builtin_amdgcn_wave_barrier();
    for (int t0 = 0; t0 < seg; t0 += 64) {
        const bool act = t0 + lane < seg;
        const int mb = act ? (int)bkt[s0 + t0 + lane] : -1;
        const unsigned long long m = hf_match_lanes<BITS>(mb);             // lanes of this group in my bin
        const unsigned long long below = m & ((1ull << lane) - 1ull);
        int pos = 0;
        if (act) pos = run[mb] + __popcll(below);
        __builtin_amdgcn_wave_barrier();
        if (act && below == 0) run[mb] += __popcll(m);                     // the first lane of each bin advances it
        __builtin_amdgcn_wave_barrier();
        if (act) {
            const int t = s0 + t0 + lane;
            st_out[pos] = t;
            if (undo_out) undo_out[t] = pos;
        }
    }
}

template <int BITS, int SEG>
static int hf_launch_sort(int B, int H, int T, int n_hashes, int NB, int32_t* st, int32_t* undo, hipStream_t stream) {
    const bool w8 = T >= HH_W8_MIN_T && T % 512 == 0;
    const size_t lds = ((T * 2 + 15) & ~15) + (size_t)((w8 ? 8 : 4) + 1) * 64 * SEG * 4;       // <= 16 KB + 9 * 320 * 4 = 27.5 KB
    if (w8)
        hipLaunchKernelGGL((lsh_sort_ids_hf_kernel<BITS, SEG, 8>), dim3(B * H * n_hashes), dim3(512), lds, stream, T, NB, st, undo);
    else
        hipLaunchKernelGGL((lsh_sort_ids_hf_kernel<BITS, SEG, 4>), dim3(B * H * n_hashes), dim3(256), lds, stream, T, NB, st, undo);
    RTTS_LAUNCH_CHECK("rtts_lsh_hash_sort_hf (sort)");
    return 0;
}

extern "C" int rtts_lsh_hash_sort_hf(const void* qk, int64_t ld_qk, const float* rotations, const uint8_t* mask, int B, int H, int T,
                                     int dh, int n_hashes, int chunk, int n_buckets, int32_t* buckets, int32_t* st, int32_t* undo,
                                     void* stream) {
    RTTS_ENTER(stream);
    RTTS_REQUIRE(qk && rotations && st, "rtts_lsh_hash_sort_hf: null pointer");
    RTTS_REQUIRE(dh == HH_DH, "rtts_lsh_hash_sort_hf: dh=%d unsupported (this build: 64)", dh);
    RTTS_REQUIRE(n_buckets >= 2 && n_buckets <= 256 && n_buckets % 2 == 0,
                 "rtts_lsh_hash_sort_hf: n_buckets=%d unsupported (even, 2 .. 256)", n_buckets);
    RTTS_REQUIRE(chunk > 0 && T > 0 && T % chunk == 0, "rtts_lsh_hash_sort_hf: sequence length (%d) must be a multiple of the chunk length (%d)",
                 T, chunk);
    RTTS_REQUIRE(T % 128 == 0 && T <= 8192, "rtts_lsh_hash_sort_hf: T=%d must be a multiple of 128 and <= 8192", T);
    RTTS_REQUIRE(B > 0 && H > 0 && n_hashes > 0 && n_hashes <= 16, "rtts_lsh_hash_sort_hf: bad B/H/n_hashes");
    RTTS_REQUIRE(ld_qk >= (int64_t)H * dh && ld_qk % 8 == 0, "rtts_lsh_hash_sort_hf: ld_qk must be >= H*dh and a multiple of 8");
    RTTS_REQUIRE(((uintptr_t)qk & 15) == 0, "rtts_lsh_hash_sort_hf: qk must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int NB = n_buckets + (mask ? 1 : 0);          // bins of the sort = stride of the round offsets
    const int half = n_buckets / 2;
#define HH_LAUNCH(C)                                                                                                              \
    hipLaunchKernelGGL((lsh_hash_hf_kernel<C>), dim3(B * H * (T / 128)), dim3(256), 0, s, (const bf16_t*)qk, ld_qk, rotations, mask, H, T, \
                       n_hashes, half, NB, buckets, st)
    // column capacity = the next power of two; the extra columns are zero padding that the argmax ignores
    if (half <= 1) HH_LAUNCH(1);
    else if (half <= 2) HH_LAUNCH(2);
    else if (half <= 4) HH_LAUNCH(4);
    else if (half <= 8) HH_LAUNCH(8);
    else if (half <= 16) HH_LAUNCH(16);
    else if (half <= 32) HH_LAUNCH(32);
    else if (half <= 64) HH_LAUNCH(64);
    else HH_LAUNCH(128);
#undef HH_LAUNCH
    RTTS_LAUNCH_CHECK("rtts_lsh_hash_sort_hf (hash)");
    if (NB <= 4) return hf_launch_sort<2, 1>(B, H, T, n_hashes, NB, st, undo, s);
    if (NB <= 8) return hf_launch_sort<3, 1>(B, H, T, n_hashes, NB, st, undo, s);
    if (NB <= 16) return hf_launch_sort<4, 1>(B, H, T, n_hashes, NB, st, undo, s);
    if (NB <= 32) return hf_launch_sort<5, 1>(B, H, T, n_hashes, NB, st, undo, s);
    if (NB <= 64) return hf_launch_sort<6, 1>(B, H, T, n_hashes, NB, st, undo, s);
    if (NB <= 128) return hf_launch_sort<7, 3>(B, H, T, n_hashes, NB, st, undo, s);
    if (NB <= 192) return hf_launch_sort<8, 3>(B, H, T, n_hashes, NB, st, undo, s);
    if (NB <= 256) return hf_launch_sort<8, 5>(B, H, T, n_hashes, NB, st, undo, s);
    return hf_launch_sort<9, 5>(B, H, T, n_hashes, NB, st, undo, s);
}
