// LDS tile layouts and row staging of the MFMA attention kernels (lsh_attn_fwd.hip, lsh_attn_bwd.hip, xattn.hip, full_attn.hip):
// the one definition of the offset functions and of the bank arithmetic behind them.  The offset functions are kept free of
// anything a host compiler does not know, so that tests/test_lds_swizzle_model.py runs the LDS banking model on the functions
// the kernels compile (tests/attn_tile_host.cpp prints their tables); the device helpers follow under __HIPCC__.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AT_HD __host__ __device__
#else
#define AT_HD
#endif

#define AT_PADB 144       // padded LDS row (bytes): 128 B of bf16 + 16 B, conflict-free ds_read_b128 of one piece from 16 rows
#define AT_SELF (-5e4f)   // logit of a shared-QK query against itself (reformer_pytorch's TOKEN_SELF_ATTN_VALUE)

// ---- row images ---------------------------------------------------------------------------------------------------
// K/Q, V and dout images: [row][128 B], no padding; the eight 16-byte pieces of a row are XOR-swizzled with
//     sw(row) = row bits (2,1) | (row bit 3 ^ row bit 1) << 2
// so that BOTH access shapes are bank-conflict free (64 banks x 4 B): ds_read_b128 of one piece from 16 rows (the MFMA
// A/B fragments) and ds_read_b64_tr_b16 of 4 consecutive rows x 64 B (the transposed fragments).  With 144-byte padded
// rows the transposed reads were 2-way conflicted (rows j and j+2 overlap in 8 banks).  An image is filled by LDS-DMA, which
// writes 8 consecutive rows in lane order: the swizzle goes on the SOURCE side (physical piece p of a row fetches p ^ sw(row)).
AT_HD constexpr int at_sw(int row) { return ((row >> 1) & 3) | ((((row >> 3) ^ (row >> 1)) & 1) << 2); }
AT_HD constexpr int at_off(int row, int piece) { return row * 128 + ((piece ^ at_sw(row)) << 4); }
// dS'^T image: [key][BS queries] bf16 (BS = 64 or 128), no padding, 8-byte granules (4 queries) XOR-swizzled by the key so that
// the ds_write_b64 of 16 consecutive keys (banks mod 32) and the transposed read of 4 consecutive keys x 64 B (banks mod 64)
// are both conflict free (the padded image was 4-way conflicted on the read side: the dQ phase ran at LDS speed / 4).
template <int BS>
AT_HD constexpr int at_ds_off(int key, int gran) {
    const int k0 = key & 1, k1 = (key >> 1) & 1, k2 = (key >> 2) & 1, k3 = (key >> 3) & 1;
    if (BS == 128) return key * 256 + ((gran ^ ((k1 << 4) | (k0 << 3) | (k1 << 2) | (k2 << 1) | k3)) << 3);
    return key * 128 + ((gran ^ ((k1 << 3) | (k0 << 2) | (k2 << 1) | k3)) << 3);
}

// ---- row staging of the epilogues: [32 rows][128 B] -----------------------------------------------------------------
// The accumulators hold a row (query / key) per lane and 4 dh values per register group, so a lane's natural store is 8 bytes
// into 16 different 128-byte rows.  Through this image a wave leaves full rows instead.  Lane (r, hh) writes the 8 bytes
// (16-byte piece p, half hh) of row r with ds_write_b64 (16 consecutive lanes = 16 rows per LDS cycle, banks mod 32: the
// 16 rows must land on the 16 distinct 8-byte slots of a 128-byte window) and the rows leave as 16-byte pieces read with
// ds_read_b128 (lane = (row & 7, piece), groups of 16 lanes = 4 rows x 4 pieces, banks mod 64: rows of equal parity must
// hold different pieces).  piece ^ (row & 7) serves both; the half is swapped in rows with bit 3 set, which the reader
// undoes for free: bit 3 of its row is the compile-time index of the read.  (A padded [32][144 B] staging was 2-way
// conflicted on both sides: 10.9 % of the LSH backward's LDS cycles.)
AT_HD constexpr int at_stg_w(int r, int piece, int hh) { return r * 128 + ((piece ^ (r & 7)) << 4) + ((hh ^ ((r >> 3) & 1)) << 3); }
AT_HD constexpr int at_stg_r(int i, int srow, int spiece) { return (i * 8 + srow) * 128 + ((spiece ^ srow) << 4); }

static_assert(at_off(8, 3) == 8 * 128 + 7 * 16 && at_ds_off<64>(5, 0) == 5 * 128 + 6 * 8 && at_ds_off<128>(2, 0) == 2 * 256 + 20 * 8, "images");
static_assert(at_stg_w(9, 0, 0) == 9 * 128 + 16 + 8 && at_stg_r(1, 3, 0) == 11 * 128 + 3 * 16, "row staging");

#if defined(__HIPCC__)
#include "rtts_common.h"

// read half of the staging: piece `spiece` of row 8 i + srow in its natural order (one ds_read_b128; i a compile-time index)
__device__ __forceinline__ uint4 at_stg_row(const unsigned char* stg, int i, int srow, int spiece) {
    const uint4 v = *reinterpret_cast<const uint4*>(stg + at_stg_r(i, srow, spiece));
    return (i & 1) ? uint4{v.z, v.w, v.x, v.y} : v;
}
// acc[dt][4 g + j] of lane (r, hh) = element (row r, dh = 32 dt + 8 g + 4 hh + j), times `mul`  ->  32 rows of 64 bf16 at
// dst + row * ld (16-byte aligned rows), through the wave-private 4 KB image `stg`: 4 ds_read_b128 + 4 16-byte write-through
// stores (8 complete rows per instruction)
__device__ __forceinline__ void at_store_rows(unsigned char* stg, const f32x16 (&acc)[2], float mul, bf16_t* dst, int64_t ld, int lane) {
    const int r = lane & 31, hh = lane >> 5, srow = lane >> 3, spiece = lane & 7;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 pk;
            pk.x = pack_bf16x2(acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul);
            pk.y = pack_bf16x2(acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul);
            *reinterpret_cast<uint2*>(stg + at_stg_w(r, dt * 4 + g, hh)) = pk;
        }
    __builtin_amdgcn_wave_barrier();
    uint4 rowv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rowv[i] = at_stg_row(stg, i, srow, spiece);
#pragma unroll
    for (int i = 0; i < 4; ++i) rtts_store16_out(dst + (size_t)(i * 8 + srow) * ld + spiece * 8, rowv[i]);
    __builtin_amdgcn_wave_barrier();
}
#endif
