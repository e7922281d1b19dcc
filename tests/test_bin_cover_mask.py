"""bin_cover_mask (csrc/sort_bin_cover.h): the 64-bit mask of the tiles of an 8 x 8 tile block that a packed rectangle covers -
what a hit lane of k_bin_scatter<false> forms before the transpose.  The header is plain C++: compiled for the host here and
checked, exhaustively, against a double loop over the block's tiles."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-gaussian-splatting_amd", "csrc")

# every rectangle with origin 0..23 and extent 1..24 in both axes against the block at tile (8, 8), in this order; then the
# records without a rectangle (bit 31) that must give 0
DRIVER = r"""
#include <cstdio>
#include "sort_bin_cover.h"
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "wb");
    if (!f) return 1;
    for (uint32_t y0 = 0; y0 < 24; ++y0)
        for (uint32_t x0 = 0; x0 < 24; ++x0)
            for (uint32_t h = 1; h <= 24; ++h)
                for (uint32_t w = 1; w <= 24; ++w) {
                    const uint64_t m = bin_cover_mask(x0 | y0 << 7 | w << 14 | h << 21, 8u, 8u);
                    fwrite(&m, sizeof m, 1, f);
                }
    const uint32_t none[3] = {0x80000000u, 0x80000007u, 0x80000000u | 9u | 9u << 7 | 3u << 14 | 3u << 21};
    for (int i = 0; i < 3; ++i) {
        const uint64_t m = bin_cover_mask(none[i], 8u, 8u);
        fwrite(&m, sizeof m, 1, f);
    }
    return fclose(f);
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cover_mask_against_a_double_loop(tmp_path):
    src, exe, out = tmp_path / "cover.cpp", tmp_path / "cover", tmp_path / "masks.bin"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    subprocess.run([str(exe), str(out)], check=True, timeout=60)
    got = np.fromfile(out, dtype=np.uint64)
    assert got.shape[0] == 24 ** 4 + 3
    assert not got[-3:].any()
    got = got[:-3].reshape(24, 24, 24, 24)                           # [y0][x0][h - 1][w - 1]
    y0, x0, h, w = np.meshgrid(np.arange(24), np.arange(24), np.arange(1, 25), np.arange(1, 25), indexing="ij")
    want = np.zeros(got.shape, np.uint64)
    for ty in range(8):                                             # the double loop: tile (8 + tx, 8 + ty) of the block
        for tx in range(8):
            inside = (x0 <= 8 + tx) & (8 + tx < x0 + w) & (y0 <= 8 + ty) & (8 + ty < y0 + h)
            want |= inside.astype(np.uint64) << np.uint64(ty * 8 + tx)
    assert np.array_equal(got, want)
    assert want.any() and (want == np.uint64(0xFFFFFFFFFFFFFFFF)).any() and (want == 0).any()
