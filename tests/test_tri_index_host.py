"""lower_tri_index of csrc/tri_index.h (plain C++, no GPU): the kernels that take one workgroup per
lower tile or super-tile decode their block index with it. For every t a grid of 2048 tile rows can
hold - tile index up to N = 131 072 - the result is a lower-triangle position, j <= i, and the
position of t, i (i + 1) / 2 + j == t. Compiled with the host compiler and a small main into a
temporary directory, as tests/test_tile_lists_host.py compiles its own."""
import os
import subprocess

from test_tile_lists_host import CSRC, host_compiler

ROWS = 2048
MAIN = r'''
#include <cstdio>
#include "tri_index.h"
int main() {  // the number of t in [0, ROWS (ROWS + 1) / 2) decoded wrongly, and the first one
    const int T = %d * (%d + 1) / 2;
    long bad = 0;
    int first = -1, last_i = -1;
    for (int t = 0; t < T; ++t) {
        int i = -1, j = -1;
        lower_tri_index(t, i, j);
        const bool ok = 0 <= j && j <= i && (long)i * (i + 1) / 2 + j == t;
        if (!ok && first < 0) first = t;
        bad += !ok;
        last_i = i;
    }
    printf("%%d %%ld %%d %%d\n", T, bad, first, last_i);
    return 0;
}
''' % (ROWS, ROWS)


def test_lower_tri_index_every_t(tmp_path):
    src = tmp_path / 'main.cpp'
    src.write_text(MAIN)
    exe = str(tmp_path / 'tri_index_main')
    subprocess.check_call([host_compiler(), '-std=c++17', '-O1', '-Wall', '-I', CSRC, str(src),
                           '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    total, bad, first, last_i = (int(x) for x in out)
    assert total == ROWS * (ROWS + 1) // 2
    assert bad == 0, 'first wrong t: {0}'.format(first)
    assert last_i == ROWS - 1
