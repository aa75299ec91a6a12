"""CPU check of the piece -> row arithmetic of the convolution form of rtts_gemm_nt (csrc/conv_taps.h, used by the kernel in
csrc/gemm_nt.hip): tests/conv_taps_host.cpp is compiled with the host compiler and walks the same constexpr helpers the kernel
calls.  For every tile family, every wave, every piece and M in {BM, BM + 64, 3 BM - 64} (tiles at m0 = 0, BM, ...; the
caller's buffer holds input rows [-2, M + 2)):
  * the union of the input rows the DMA pieces address is [m0 - 2, m0 + BM + 2) clipped to the caller's rows -- nothing outside;
  * the pieces cover the LDS image (a repeated piece rewrites the same bytes), and a row the tile reads holds ITS input row;
  * every image a stage reads was issued at least two stages earlier and is covered by a counted wait by then;
  * under the image's swizzle key the A fragment reads are free of LDS bank conflicts at every tap shift."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reformer-tts_amd", "csrc")
TAPS = 5


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("conv_taps") / "conv_taps_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "conv_taps_host.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    fams, pieces, keys, sched = [], {}, [], {}
    for line in out.splitlines():
        v = line.split()
        if v[0] == "K":
            keys = [int(x) for x in v[1:]]
        elif v[0] == "S":
            sched[int(v[1])] = (int(v[2]), int(v[3]))
        elif v[0] == "F":
            fams.append(tuple(int(x) for x in v[1:]))
        else:
            bm, bn, nw, M, m0, w, t = (int(x) for x in v[1:8])
            rows = [int(x) for x in v[8:]]
            pieces.setdefault((bm, bn, nw, M, m0), []).append((w, t, rows[:8], rows[8:]))
    return fams, pieces, keys, sched


def test_family_table_is_the_kernels(plan):
    """conv_taps.h lists exactly the tile families gn_pick chooses from, each passes the geometry the kernel asserts, and the
    form is offered exactly up to the channel-block count whose images, with the weight ring, fit the CU's 160 KB of LDS"""
    fams = plan[0]
    src = open(os.path.join(CSRC, "gemm_nt.hip")).read()
    cand = re.search(r"gn_cand\[GN_NCAND\]\[3\] = \{(.*?)\};", src).group(1)
    cand = [tuple(int(x) for x in c.split(",")) for c in re.findall(r"\{([^{}]*)\}", cand)]
    assert [(bm, bn) for bm, bn, _ in cand] == [(f[0], f[1]) for f in fams]
    for bm, bn, nw, npieces, pa, image_rows, ok, max_cpt in fams:
        assert ok == 1, (bm, bn)
        assert image_rows == 8 * npieces and bm + 4 <= image_rows < bm + 12 and pa * nw >= npieces
        assert max_cpt >= 1
        assert max_cpt * image_rows * 128 + 3 * bn * 128 <= 160 * 1024 < (max_cpt + 1) * image_rows * 128 + 3 * bn * 128
    assert {(f[0], f[1]): f[7] for f in fams}[(128, 64)] == 8           # the encoder prenet's 512 channels fit


def test_pieces_cover_the_halo_image_and_nothing_else(plan):
    fams, pieces, _, sched = plan
    assert len(pieces) == sum(len(range(0, M, f[0])) for f in fams for M in (f[0], f[0] + 64, 3 * f[0] - 64))
    pa_of = {(f[0], f[2]): f[4] for f in fams}
    rows_of = {f[0]: f[5] for f in fams}
    for (bm, bn, nw, M, m0), plist in pieces.items():
        assert len(plist) == nw * pa_of[(bm, nw)]                    # every wave issues the same number of pieces
        want = set(range(max(m0 - 2, -2), min(m0 + bm + 2, M + 2)))
        got = set()
        lds = {}
        for w, t, lds_rows, src_rows in plist:
            got.update(src_rows)
            for j, srow in zip(lds_rows, src_rows):
                assert lds.setdefault(j, srow) == srow               # a repeated piece writes the same input row to the same place
        assert got == want, (bm, bn, M, m0, sorted(got - want), sorted(want - got))
        assert sorted(lds) == list(range(rows_of[bm]))
        # a tap that reads at shift u reads image rows [u, u + BM); rows beyond the caller's buffer exist only for a partial last
        # tile, whose outputs nobody keeps
        for u in range(TAPS):
            for j in range(u, u + bm):
                if m0 - 2 + j > M + 1:
                    continue
                assert lds[j] == m0 - 2 + j, (bm, M, m0, u, j)       # the row holds its own input row
    # image cb is first read by K stage cb (tap 0): issued at least two stages earlier, and covered by a counted wait by then
    assert sorted(sched) == list(range(10))
    for cb, (issue, ready) in sched.items():
        assert cb - issue >= 2 and ready <= cb


# the four 16-lane groups in which the LDS serves one ds_read_b128 of a 64-lane wave: only lanes of one group can conflict
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)), list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def test_fragment_reads_are_conflict_free_at_every_tap_shift(plan):
    """Lane 16 g + r reads chunk (g + 4 ks) ^ key(row) of image row = base + r + u (128-byte rows: 64 banks of 4 bytes hold two
    rows, the odd one in banks 32..63).  For every tap shift u, k32-step ks and 16-row tile base, the 16 lanes of each group
    must touch 16 distinct 16-byte slots of the 256-byte bank line.  The plain form's key (row >> 1) & 7 fails this for
    u = 1, 2, 3 (checked here too, so that the test is known to see a conflict)."""
    keys = plan[2]
    assert sorted(sum(B128_GROUPS, [])) == list(range(64)) and len(keys) == 64

    def conflicts(key, u):
        bad = 0
        for base in (0, 16, 32):
            for ks in (0, 1):
                for lanes in B128_GROUPS:
                    slots = set()
                    for lane in lanes:
                        g, r = lane >> 4, lane & 15
                        row = base + r + u
                        slots.add((row & 1) * 8 + ((g + 4 * ks) ^ key(row)))
                    bad += 16 - len(slots)
        return bad

    for u in range(TAPS):
        assert conflicts(lambda row: keys[row], u) == 0, u
    assert all(0 <= k < 8 for k in keys)
    # the key depends on the row inside an 8-row piece alone: one per-lane source swizzle serves every piece of every wave
    assert all(keys[row] == keys[row % 8] for row in range(64))
    plain = [conflicts(lambda row: (row >> 1) & 7, u) for u in range(TAPS)]
    assert plain[0] == 0 and plain[4] == 0 and all(plain[u] > 0 for u in (1, 2, 3))
