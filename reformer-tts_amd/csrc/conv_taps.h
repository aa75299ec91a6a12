// Piece -> row arithmetic of the convolution form of rtts_gemm_nt's main loop (gemm_nt.hip, MODE 3), kept free of anything
// a host compiler does not know so that tests/test_conv_taps_cpu.py can walk it without a GPU.
//
// A workgroup of NW waves on a BM-row tile keeps the input rows [m0 - 2, m0 + BM + 2) of ALL its 64-channel blocks in LDS --
// one image per channel block ("image rows" j, image row j = input row m0 - 2 + j) -- and reads every image at five row
// shifts (the taps).  K keeps the order of the plain loop (tap-major: stage s = tap s / cpt, channel block s % cpt), so the
// fp32 sums are the plain loop's, bit for bit; the images arrive with the stages of tap 0 (image cb in the DMA group of stage
// cb) and the stages of taps 1..4 bring in the weight tile only.
// An image is gn_conv_pieces(BM) 1-KB DMA pieces (8 rows of 128 bytes); every wave issues gn_conv_pa(BM, NW) pieces per image,
// piece t of wave w = image piece min(w + NW t, pieces - 1): the surplus ones repeat the last piece (same source, same
// destination, same bytes), so that all waves count the same number of DMA instructions.  Image rows > BM + 3 are never read;
// the lanes that would fetch them fetch the last row the tile may read instead (input row min(m0 + BM + 1, M + 1)): no address
// is formed beyond what the plain loop reads.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GN_CT_HD __host__ __device__
#else
#define GN_CT_HD
#endif

#define GN_CONV_TAPS 5
#define GN_CONV_NST 3          // weight-ring depth of the convolution form

// 8-row pieces of one image (the last one holds the 4 halo rows behind the tile), rows and bytes of an image
GN_CT_HD constexpr int gn_conv_pieces(int bm) { return (bm + 4 + 7) / 8; }
GN_CT_HD constexpr int gn_conv_image_rows(int bm) { return 8 * gn_conv_pieces(bm); }
GN_CT_HD constexpr int gn_conv_image_bytes(int bm) { return gn_conv_image_rows(bm) * 128; }
// A pieces per wave and image
GN_CT_HD constexpr int gn_conv_pa(int bm, int nw) { return (gn_conv_pieces(bm) + nw - 1) / nw; }
// image piece that piece t of wave w fills
GN_CT_HD constexpr int gn_conv_piece(int bm, int nw, int w, int t) {
    return (w + nw * t) < gn_conv_pieces(bm) - 1 ? (w + nw * t) : gn_conv_pieces(bm) - 1;
}
// image row (= LDS row) that lane row `lr` (lane >> 3, 0..7) of piece `t` of wave `w` writes
GN_CT_HD constexpr int gn_conv_lds_row(int bm, int nw, int w, int t, int lr) { return 8 * gn_conv_piece(bm, nw, w, t) + lr; }
// last image row a tile at m0 of a problem of M rows may fetch: the tile's own halo (BM + 3) and the caller's (input row M + 1)
GN_CT_HD constexpr int gn_conv_last_row(int bm, int m0, int M) { return (M + 3 - m0) < (bm + 3) ? (M + 3 - m0) : (bm + 3); }
// image row whose DATA that lane fetches: its own while the tile may read it, else the last one it may
GN_CT_HD constexpr int gn_conv_src_row(int bm, int nw, int w, int t, int lr, int m0, int M) {
    return gn_conv_lds_row(bm, nw, w, t, lr) < gn_conv_last_row(bm, m0, M) ? gn_conv_lds_row(bm, nw, w, t, lr) : gn_conv_last_row(bm, m0, M);
}
// pieces t < gn_conv_plain_pieces() of every wave lie wholly inside the rows every tile reads (8 p + 7 <= BM + 3) and are not
// repeated: their source is the wave's piece 0 moved on by 8 NW t rows; the others take a per-lane source row (gn_conv_src_row)
GN_CT_HD constexpr int gn_conv_plain_pieces(int bm, int nw) { return ((bm - 4) / 8 + 1) / nw; }
// XOR swizzle of the image's 16-byte chunks (128-byte rows: two rows per 256-byte bank line, eight chunks each), applied on the
// source side of the DMA and again by the fragment reads.  A ds_read_b128 is served in four groups of 16 lanes; with lane =
// 16 g + r reading chunk g of tile row r, a group holds rows r in {0..3, 12..15} of chunk g and rows {4..11} of chunk g ^ 1.
// A tap reads rows r + u, so the key must keep those 16 accesses on 16 distinct (row parity, chunk) slots for EVERY shift
// u, not only u = 0: (row >> 1) & 7 -- the plain form's key -- is 2-way for u = 1, 2, 3; 2 ((row >> 1) & 3) is conflict-free for
// every shift (rows of one parity: the key repeats with period 4 in row >> 1, and rows k, k + 4 of the 8 sit in different halves
// {g, g ^ 1} of the group).  tests/test_conv_taps_cpu.py walks all shifts and groups.
GN_CT_HD constexpr int gn_conv_swz(int row) { return ((row >> 1) & 3) << 1; }
// Stages are the K stages of the tile (stage s = tap s / cpt, channel block s % cpt); image cb is first read by stage cb.
//   issue: the DMA group of stage X (its weight pieces, and image X when X < cpt) goes out under the second MFMA burst of stage
//          X - NST and the first burst of stage X - NST + 1 (groups 0 .. NST - 1: before the loop);
//   ready: the counted wait in front of the barrier that ends stage X - 1 covers group X (returns are in order), so the first
//          fragment read that may touch image X is the one of stage X, issued behind that barrier.
GN_CT_HD constexpr int gn_conv_issue_stage(int cb) { return cb - GN_CONV_NST + 1; }
GN_CT_HD constexpr int gn_conv_ready_stage(int cb) { return cb; }
// LDS of the form: cpt images + the weight ring; the form serves a convolution only where this fits the CU's 160 KB
GN_CT_HD constexpr long gn_conv_lds_bytes(int bm, int bn, int cpt) { return (long)cpt * gn_conv_image_bytes(bm) + (long)GN_CONV_NST * bn * 128; }
GN_CT_HD constexpr bool gn_conv_fits(int bm, int bn, int cpt) { return gn_conv_lds_bytes(bm, bn, cpt) <= 160 * 1024; }

// the tile families of rtts_gemm_nt (gn_cand): BM, BN, waves along M, waves in all
struct GnConvFamily { int bm, bn, wm, nw; };
#define GN_CONV_NFAMILY 5
constexpr GnConvFamily gn_conv_family[GN_CONV_NFAMILY] = {{256, 256, 4, 8}, {192, 128, 4, 8}, {256, 128, 4, 8}, {96, 64, 2, 4}, {128, 64, 2, 4}};

// what the kernel relies on, for one family
GN_CT_HD constexpr bool gn_conv_family_ok(int bm, int nw) {
    return gn_conv_pa(bm, nw) * nw >= gn_conv_pieces(bm)                        // the waves' pieces cover the image
        && gn_conv_plain_pieces(bm, nw) >= gn_conv_pa(bm, nw) - 1                 // at most the last piece of a wave is clamped / repeated
        && (8 * nw) % 8 == 0 && nw % 2 == 0                                       // the swizzle key does not depend on the piece
        && gn_conv_issue_stage(GN_CONV_NST) + 2 <= gn_conv_ready_stage(GN_CONV_NST);   // issued two stages before the first read
}
