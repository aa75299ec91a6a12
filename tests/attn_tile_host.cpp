// Host-side walk of csrc/attn_tile.h for tests/test_lds_swizzle_model.py: prints the offset functions the attention kernels
// compile, over the whole domain the bank model walks -- one line each:
//   O row sw off(piece 0..7)          rows 0..255 of a [row][128 B] image
//   D bs key off(granule 0..bs/4-1)   keys 0..255 of the dS^T image, bs = 64 and 128 queries per key row
//   W r piece off(hh 0) off(hh 1)     staging write, 32 rows x 8 pieces x 2 halves
//   R i srow off(spiece 0..7)         staging read, 4 x 8 x 8
#include <cstdio>

#include "attn_tile.h"

template <int BS>
static void ds_rows() {
    for (int key = 0; key < 256; ++key) {
        std::printf("D %d %d", BS, key);
        for (int g = 0; g < BS / 4; ++g) std::printf(" %d", at_ds_off<BS>(key, g));
        std::printf("\n");
    }
}

int main() {
    for (int row = 0; row < 256; ++row) {
        std::printf("O %d %d", row, at_sw(row));
        for (int p = 0; p < 8; ++p) std::printf(" %d", at_off(row, p));
        std::printf("\n");
    }
    ds_rows<64>();
    ds_rows<128>();
    for (int r = 0; r < 32; ++r)
        for (int p = 0; p < 8; ++p) std::printf("W %d %d %d %d\n", r, p, at_stg_w(r, p, 0), at_stg_w(r, p, 1));
    for (int i = 0; i < 4; ++i)
        for (int srow = 0; srow < 8; ++srow) {
            std::printf("R %d %d", i, srow);
            for (int sp = 0; sp < 8; ++sp) std::printf(" %d", at_stg_r(i, srow, sp));
            std::printf("\n");
        }
    return 0;
}
