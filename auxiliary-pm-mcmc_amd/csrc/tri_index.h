// Index t of the lower triangle, rows in order (0,0), (1,0), (1,1), (2,0), .. -> (i, j), j <= i,
// with i (i + 1) / 2 + j = t: the grids of the kernels that take one workgroup per lower tile or
// super-tile. The fp64 square root lands within one of the row; the two loops correct it in
// integers. Plain C++ as well (tests/test_tri_index_host.py walks every t a grid can hold).
#pragma once
#include <math.h>

#include "apm_hd.h"

APM_HD inline void lower_tri_index(int t, int& i, int& j) {
    int r = (int)floor((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    i = r;
    j = t - r * (r + 1) / 2;
}
