// Host-side walk of csrc/conv_taps.h for tests/test_conv_taps_cpu.py: prints, for every tile family, what the convolution form
// of rtts_gemm_nt issues for one image (every channel block's image is issued alike) -- one line per (family, M, tile, wave, piece):
//   P bm bn nw M m0 wave t  lds_row[0..7]  src_input_row[0..7]
// (input rows are counted from the caller's row 0: image row j of the tile at m0 is input row m0 - 2 + j), one line
//   F bm bn nw pieces pieces_per_wave image_rows ok max_cpt
// per family with the geometry the kernel static_asserts and the largest channel-block count whose images fit LDS, one line
//   S cb issue_stage ready_stage
// per channel block 0..9 (image cb is first read by K stage cb), and one line
//   K key(0) .. key(63)
// with the swizzle key of image rows 0..63.
#include <cstdio>

#include "conv_taps.h"

int main() {
    std::printf("K");
    for (int row = 0; row < 64; ++row) std::printf(" %d", gn_conv_swz(row));
    std::printf("\n");
    for (int cb = 0; cb < 10; ++cb) std::printf("S %d %d %d\n", cb, gn_conv_issue_stage(cb), gn_conv_ready_stage(cb));
    for (int f = 0; f < GN_CONV_NFAMILY; ++f) {
        const GnConvFamily& F = gn_conv_family[f];
        int max_cpt = 0;
        while (gn_conv_fits(F.bm, F.bn, max_cpt + 1)) ++max_cpt;
        std::printf("F %d %d %d %d %d %d %d %d\n", F.bm, F.bn, F.nw, gn_conv_pieces(F.bm), gn_conv_pa(F.bm, F.nw), gn_conv_image_rows(F.bm),
                    gn_conv_family_ok(F.bm, F.nw) ? 1 : 0, max_cpt);
        const int Ms[3] = {F.bm, F.bm + 64, 3 * F.bm - 64};
        for (int M : Ms)
            for (int m0 = 0; m0 < M; m0 += F.bm)
                for (int w = 0; w < F.nw; ++w)
                    for (int t = 0; t < gn_conv_pa(F.bm, F.nw); ++t) {
                        std::printf("P %d %d %d %d %d %d %d ", F.bm, F.bn, F.nw, M, m0, w, t);
                        for (int lr = 0; lr < 8; ++lr) std::printf(" %d", gn_conv_lds_row(F.bm, F.nw, w, t, lr));
                        for (int lr = 0; lr < 8; ++lr) std::printf(" %d", m0 - 2 + gn_conv_src_row(F.bm, F.nw, w, t, lr, m0, M));
                        std::printf("\n");
                    }
    }
    return 0;
}
