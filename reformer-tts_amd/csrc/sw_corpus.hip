// One vocoder training batch drawn from a device-resident corpus, one launch (rtts_sw_draw_segments of include/rtts.h): the
// fixed-length crop of SpectrogramToSpeechDataset.__getitem__ (reference dataset/interface.py:64-97) for every slot of a batch,
// with the utterance and the hop decided on the device, written in the row layout SqueezeWave's training step consumes.
//
// Grid (tiles, B): the workgroups of slot b all repeat the same few scalar reads (cursor, order, the two offset pairs) and the
// same hash, so they agree on (utterance, hop) without talking to each other; nothing a workgroup reads is written by the
// launch.  The first DS_AUDIO_TILE-sample tiles of a slot copy audio, the rest transpose mel:
//   audio  a straight copy of S samples from an arbitrary sample offset.  The destination of a vector is 16-byte aligned; the
//          source is only element aligned, and one test per workgroup (every vector of a tile shares its first one's alignment)
//          picks 16-, 8- or 4-byte loads for f32 and 8-, 4- or 2-byte loads for int16.  The vector that straddles the end of the
//          utterance, and a destination that is not 16-byte aligned, take the guarded element path;
//   mel    source (n_mel, ld_mel) is contiguous along frames, destination (frames, n_mel) along channels: a wave reads 64
//          consecutive frames of one channel (256 contiguous bytes), the tile goes through LDS with an odd row pitch -- the 32
//          lanes of a ds_write group (32 frames, one channel) and of a ds_read group (consecutive channels) both fall on 32
//          different banks -- and leaves as consecutive words of the output rows (one contiguous run when ld_mel_rows == n_mel).
// No atomics; every output word is written exactly once and depends on the arguments alone.
#include "rtts_common.h"

#define DS_THREADS 256
#define DS_AUDIO_TILE 4096        // samples of one audio workgroup: 4 vectors of 4 per lane
#define DS_MEL_TILE 64            // frames of one mel workgroup: one wave's width
#define DS_MAX_MEL 128

struct DsPick {
    int32_t u, h;        // u = -1: nothing to read, the segment is zeros
    int64_t a0, n;       // first sample of the crop in `audio`, samples the crop may read (0 .. S)
    int64_t f0, t;       // first column of the crop in `mel`, frames the crop may read (0 .. seg_frames)
};

// (utterance, hop) of slot b and the bounds every read of the slot is held to
__device__ __forceinline__ DsPick ds_pick(int b, int64_t n_audio, const int64_t* __restrict__ so, int64_t ld_mel,
                                          const int64_t* __restrict__ fo, int n_utt, const int32_t* __restrict__ order, int n_order,
                                          const int64_t* __restrict__ state, uint32_t seed, const int32_t* __restrict__ picks_in,
                                          int seg_frames, int hop) {
    DsPick p = {-1, 0, 0, 0, 0, 0};
    const int64_t S = (int64_t)seg_frames * hop;
    int64_t u, h = -1, i = 0;
    if (picks_in) {
        u = picks_in[2 * b];
        h = picks_in[2 * b + 1];
    } else {
        i = state[0] + b;
        int64_t r = i % n_order;
        if (r < 0) r += n_order;
        u = order[r];
    }
    if (u < 0 || u >= n_utt) return p;
    const int64_t s0 = so[u], s1 = so[u + 1], c0 = fo[u], c1 = fo[u + 1];
    // tables that point outside the buffers are treated like an utterance that does not exist
    if (s0 < 0 || s1 < s0 || s1 > n_audio || c0 < 0 || c1 < c0 || c1 > ld_mel) return p;
    const int64_t N = s1 - s0, T = c1 - c0;
    if (!picks_in) {
        h = 0;
        if (N >= S) {
            const uint64_t hops = (uint64_t)((N - S) / hop) + 1;            // max_hop + 1
            h = (int64_t)(((uint64_t)rtts_drop_hash(seed + (uint32_t)state[1], (uint32_t)i) * hops) >> 32);
        }
    }
    if (h < 0 || h > 0x7fffffff) return p;
    p.u = (int32_t)u;
    p.h = (int32_t)h;
    const int64_t skip = h * hop;
    p.a0 = s0 + skip;
    p.n = N - skip < 0 ? 0 : (N - skip > S ? S : N - skip);
    p.f0 = c0 + h;
    p.t = T - h < 0 ? 0 : (T - h > seg_frames ? seg_frames : T - h);
    return p;
}

template <int FMT>
__device__ __forceinline__ float ds_sample(const void* __restrict__ audio, int64_t i) {
    if (FMT == 0) return static_cast<const float*>(audio)[i];
    return (float)static_cast<const int16_t*>(audio)[i] * (1.f / 32768.f);
}

// four consecutive samples from element i, by the widest loads `align` (bytes, a power of two <= 16) allows
template <int FMT>
__device__ __forceinline__ float4 ds_load4(const void* __restrict__ audio, int64_t i, int align) {
    if (FMT == 0) {
        const float* s = static_cast<const float*>(audio) + i;
        if (align >= 16) return *reinterpret_cast<const float4*>(s);
        if (align >= 8) {
            const float2 lo = *reinterpret_cast<const float2*>(s), hi = *reinterpret_cast<const float2*>(s + 2);
            return make_float4(lo.x, lo.y, hi.x, hi.y);
        }
        return make_float4(s[0], s[1], s[2], s[3]);
    }
    const int16_t* s = static_cast<const int16_t*>(audio) + i;
    short4v v;
    if (align >= 8) {
        v = *reinterpret_cast<const short4v*>(s);
    } else if (align >= 4) {
        const uint32_t lo = *reinterpret_cast<const uint32_t*>(s), hi = *reinterpret_cast<const uint32_t*>(s + 2);
        v = short4v{(short)(lo & 0xffffu), (short)(lo >> 16), (short)(hi & 0xffffu), (short)(hi >> 16)};
    } else {
        v = short4v{s[0], s[1], s[2], s[3]};
    }
    const float k = 1.f / 32768.f;
    return make_float4((float)v.x * k, (float)v.y * k, (float)v.z * k, (float)v.w * k);
}

template <int FMT>
__global__ __launch_bounds__(DS_THREADS) void sw_draw_segments_kernel(
    const void* __restrict__ audio, int64_t n_audio, const int64_t* __restrict__ so, const float* __restrict__ mel, int64_t ld_mel,
    const int64_t* __restrict__ fo, int n_utt, const int32_t* __restrict__ order, int n_order, const int64_t* __restrict__ state,
    uint32_t seed, const int32_t* __restrict__ picks_in, int seg_frames, int hop, int n_mel, int audio_tiles,
    float* __restrict__ audio_rows, float* __restrict__ mel_rows, int64_t ld_rows, int32_t* __restrict__ picks_out) {
    __shared__ float tile[DS_MEL_TILE * (DS_MAX_MEL + 1)];
    const int b = blockIdx.y, tid = threadIdx.x;
    const DsPick p = ds_pick(b, n_audio, so, ld_mel, fo, n_utt, order, n_order, state, seed, picks_in, seg_frames, hop);
    const int64_t S = (int64_t)seg_frames * hop;
    if (blockIdx.x == 0 && tid == 0) {
        picks_out[2 * b] = p.u;
        picks_out[2 * b + 1] = p.h;
    }

    if ((int)blockIdx.x < audio_tiles) {
        const int64_t j0 = (int64_t)blockIdx.x * DS_AUDIO_TILE;
        const int64_t j1 = j0 + DS_AUDIO_TILE < S ? j0 + DS_AUDIO_TILE : S;
        float* dst = audio_rows + (int64_t)b * S;
        const int esz = FMT == 0 ? 4 : 2;
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            // alignment of the source of every vector of the tile: the lowest set bit of its first one's address, up to 16
            const uintptr_t sa = reinterpret_cast<uintptr_t>(audio) + (uintptr_t)(p.a0 + j0) * esz;
            const int align = (int)((sa | 16) & (~(sa | 16) + 1));
            const int64_t jv = j0 + ((j1 - j0) & ~(int64_t)3);                // vectors cover [j0, jv)
            for (int64_t j = j0 + 4 * tid; j < jv; j += 4 * DS_THREADS) {
                float4 v;
                if (j + 4 <= p.n) {
                    v = ds_load4<FMT>(audio, p.a0 + j, align);
                } else {
                    v.x = j < p.n ? ds_sample<FMT>(audio, p.a0 + j) : 0.f;
                    v.y = j + 1 < p.n ? ds_sample<FMT>(audio, p.a0 + j + 1) : 0.f;
                    v.z = j + 2 < p.n ? ds_sample<FMT>(audio, p.a0 + j + 2) : 0.f;
                    v.w = j + 3 < p.n ? ds_sample<FMT>(audio, p.a0 + j + 3) : 0.f;
                }
                *reinterpret_cast<float4*>(dst + j) = v;
            }
            for (int64_t j = jv + tid; j < j1; j += DS_THREADS) dst[j] = j < p.n ? ds_sample<FMT>(audio, p.a0 + j) : 0.f;
        } else {
            for (int64_t j = j0 + tid; j < j1; j += DS_THREADS) dst[j] = j < p.n ? ds_sample<FMT>(audio, p.a0 + j) : 0.f;
        }
        return;
    }

    const int t0 = ((int)blockIdx.x - audio_tiles) * DS_MEL_TILE;
    const int nt = seg_frames - t0 < DS_MEL_TILE ? seg_frames - t0 : DS_MEL_TILE;     // frames of this tile
    const int pitch = n_mel | 1;
    const int lane = tid & 63, wave = tid >> 6;
    if (lane < nt) {
        const bool live = t0 + lane < p.t;
        const float* src = mel + p.f0 + t0 + lane;
        for (int m = wave; m < n_mel; m += DS_THREADS / 64) tile[lane * pitch + m] = live ? src[(int64_t)m * ld_mel] : 0.f;
    }
    __syncthreads();
    float* dst = mel_rows + ((int64_t)b * seg_frames + t0) * ld_rows;
    const int count = nt * n_mel;
    for (int e = tid; e < count; e += DS_THREADS) {
        const int t = e / n_mel, m = e - t * n_mel;
        dst[(int64_t)t * ld_rows + m] = tile[t * pitch + m];
    }
}

extern "C" int rtts_sw_draw_segments(const void* audio, int in_format, int64_t n_audio, const int64_t* sample_offsets, const float* mel,
                                     int64_t ld_mel, const int64_t* frame_offsets, int n_utt, const int32_t* order, int n_order,
                                     const int64_t* state, uint32_t seed, const int32_t* picks_in, int B, int seg_frames, int hop, int C,
                                     int n_mel, float* audio_rows, float* mel_rows, int64_t ld_mel_rows, int32_t* picks_out, void* stream) {
    RTTS_REQUIRE(audio, "rtts_sw_draw_segments: audio is a null pointer");
    RTTS_REQUIRE(sample_offsets, "rtts_sw_draw_segments: sample_offsets is a null pointer");
    RTTS_REQUIRE(mel, "rtts_sw_draw_segments: mel is a null pointer");
    RTTS_REQUIRE(frame_offsets, "rtts_sw_draw_segments: frame_offsets is a null pointer");
    RTTS_REQUIRE(audio_rows, "rtts_sw_draw_segments: audio_rows is a null pointer");
    RTTS_REQUIRE(mel_rows, "rtts_sw_draw_segments: mel_rows is a null pointer");
    RTTS_REQUIRE(picks_out, "rtts_sw_draw_segments: picks_out is a null pointer");
    RTTS_REQUIRE(picks_in || order, "rtts_sw_draw_segments: order is a null pointer (and there is no picks_in to replace the draw)");
    RTTS_REQUIRE(picks_in || state, "rtts_sw_draw_segments: state is a null pointer (and there is no picks_in to replace the draw)");
    RTTS_REQUIRE(in_format == 0 || in_format == 1, "rtts_sw_draw_segments: in_format must be 0 (f32) or 1 (int16 mono), got %d", in_format);
    RTTS_REQUIRE(B >= 1 && B <= 65535, "rtts_sw_draw_segments: B must be in 1..65535 (got %d)", B);
    RTTS_REQUIRE(seg_frames >= 1, "rtts_sw_draw_segments: seg_frames must be positive (got %d)", seg_frames);
    RTTS_REQUIRE(hop >= 1, "rtts_sw_draw_segments: hop must be positive (got %d)", hop);
    RTTS_REQUIRE(C >= 1, "rtts_sw_draw_segments: C must be positive (got %d)", C);
    RTTS_REQUIRE(n_mel >= 1 && n_mel <= DS_MAX_MEL, "rtts_sw_draw_segments: n_mel must be in 1..%d (got %d)", DS_MAX_MEL, n_mel);
    const int64_t S = (int64_t)seg_frames * hop;
    RTTS_REQUIRE(S <= ((int64_t)1 << 40), "rtts_sw_draw_segments: seg_frames * hop = %lld samples is too long a segment", (long long)S);
    RTTS_REQUIRE(S % C == 0, "rtts_sw_draw_segments: seg_frames * hop = %lld is not a multiple of C = %d", (long long)S, C);
    RTTS_REQUIRE(picks_in || n_order >= 1, "rtts_sw_draw_segments: n_order must be positive when the batch is drawn (got %d)", n_order);
    RTTS_REQUIRE(ld_mel_rows >= n_mel, "rtts_sw_draw_segments: ld_mel_rows = %lld is smaller than n_mel = %d", (long long)ld_mel_rows, n_mel);
    RTTS_REQUIRE(n_utt >= 1, "rtts_sw_draw_segments: n_utt must be positive (got %d)", n_utt);
    RTTS_REQUIRE(n_audio >= 0, "rtts_sw_draw_segments: n_audio must not be negative (got %lld)", (long long)n_audio);
    RTTS_REQUIRE(ld_mel >= 0, "rtts_sw_draw_segments: ld_mel must not be negative (got %lld)", (long long)ld_mel);
    const int64_t audio_tiles = (S + DS_AUDIO_TILE - 1) / DS_AUDIO_TILE;
    const int64_t mel_tiles = ((int64_t)seg_frames + DS_MEL_TILE - 1) / DS_MEL_TILE;
    RTTS_REQUIRE(audio_tiles + mel_tiles <= 0x7fffffff, "rtts_sw_draw_segments: seg_frames = %d is too long a segment for one launch", seg_frames);
    RTTS_ENTER(stream);
    const dim3 grid((unsigned)(audio_tiles + mel_tiles), (unsigned)B), block(DS_THREADS);
    if (in_format == 0)
        hipLaunchKernelGGL(sw_draw_segments_kernel<0>, grid, block, 0, (hipStream_t)stream, audio, n_audio, sample_offsets, mel, ld_mel,
                           frame_offsets, n_utt, order, n_order, state, seed, picks_in, seg_frames, hop, n_mel, (int)audio_tiles, audio_rows,
                           mel_rows, ld_mel_rows, picks_out);
    else
        hipLaunchKernelGGL(sw_draw_segments_kernel<1>, grid, block, 0, (hipStream_t)stream, audio, n_audio, sample_offsets, mel, ld_mel,
                           frame_offsets, n_utt, order, n_order, state, seed, picks_in, seg_frames, hop, n_mel, (int)audio_tiles, audio_rows,
                           mel_rows, ld_mel_rows, picks_out);
    RTTS_LAUNCH_CHECK("rtts_sw_draw_segments");
    return 0;
}
