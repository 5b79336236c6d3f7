"""xcd_remap and update_item of csrc/update_item.h (plain C++, no GPU): the order in which every
update launch, the u-path and the bulk panel rows deal their work items to workgroups, and the
decode of a launch that fuses the diagonal step. Compiled with the host compiler and a small main
into a temporary directory, as tests/test_tri_index_host.py compiles its own; the main only prints,
the properties are checked here."""
import signal
import subprocess

import pytest

from test_tile_lists_host import CSRC, host_compiler

TOTALS = range(1, 601)  # every remainder total % 8 many times over; holds 27, 54 and 110
NTILES, NCHAINS = (1, 2, 5), (1, 3, 8, 9)
MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "update_item.h"
int main(int argc, char** argv) {
    if (argc > 1) {  // the work item of one workgroup: "fused b t"
        const UpdateItem it = update_item(atol(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        printf("%d %d %d\n", (int)it.fused, it.b, it.t);
        return 0;
    }
    for (long total = 1; total <= 600; ++total) {  // one line per total: xcd_remap(0 .. total-1)
        for (long L = 0; L < total; ++L) printf("%ld ", xcd_remap(L, total));
        printf("\n");
    }
    const int nts[] = {1, 2, 5}, ncs[] = {1, 3, 8, 9};
    for (int nt : nts)  // one line per grid: "fused.b.t" of every workgroup
        for (int nc : ncs)
            for (int fused = 0; fused < 2; ++fused) {
                for (long blk = 0; blk < (long)nt * nc; ++blk) {
                    const UpdateItem it = update_item(blk, fused, nt, nc);
                    printf("%d.%d.%d ", (int)it.fused, it.b, it.t);
                }
                printf("\n");
            }
    return 0;
}
'''


@pytest.fixture(scope='module')
def item_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp('update_item')
    src = d / 'main.cpp'
    src.write_text(MAIN)
    exe = str(d / 'update_item_main')
    # (no -DNDEBUG: the header's host-side checks are part of what runs)
    subprocess.check_call([host_compiler(), '-std=c++17', '-O1', '-Wall', '-I', CSRC, str(src),
                           '-o', exe])
    return exe


@pytest.fixture(scope='module')
def lines(item_bin):
    out = subprocess.run([item_bin], capture_output=True, text=True, check=True).stdout
    return out.split('\n')


def test_xcd_remap_is_a_permutation_in_eight_even_contiguous_ranges(lines):
    assert {27, 54, 110} <= set(TOTALS)  # the totals tests/test_batch_counts_host.py derives
    for total, line in zip(TOTALS, lines):
        w = [int(t) for t in line.split()]
        assert sorted(w) == list(range(total)), total
        sizes = []
        for x in range(8):  # the workgroups of XCD x, in dispatch order: one contiguous range
            mine = w[x::8]
            assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True, (total, x)
            sizes.append(len(mine))
        assert max(sizes) - min(sizes) <= 1, (total, sizes)


def test_update_item_deals_every_chain_and_entry_once(lines):
    grids = [(nt, nc, fused) for nt in NTILES for nc in NCHAINS for fused in (0, 1)]
    rows = lines[len(TOTALS):len(TOTALS) + len(grids)]
    assert len(rows) == len(grids)
    for (nt, nc, fused), line in zip(grids, rows):
        items = [tuple(int(x) for x in t.split('.')) for t in line.split()]
        assert len(items) == nt * nc
        assert sorted((b, t) for _, b, t in items) == [(b, t) for b in range(nc)
                                                       for t in range(nt)], (nt, nc, fused)
        for blk, (f, b, t) in enumerate(items):
            assert f == (1 if fused and blk < nc else 0), (nt, nc, fused, blk)
            if f:  # the first nchains workgroups: entry 0 of chain blk
                assert (b, t) == (blk, 0), (nt, nc, fused, blk)
            elif fused:  # entry 0 is the fused workgroups' alone
                assert t >= 1, (nt, nc, fused, blk)


def test_one_entry_fused_grid_never_reaches_the_other_branch(item_bin):
    """ntiles == 1 with the fused flag: the grid above ran to its end, so no workgroup of it took
    the branch that divides by nt = ntiles - 1 = 0, which the header's host-side check refuses.
    That the check is compiled in is shown on a workgroup past that grid: it aborts."""
    ok = subprocess.run([item_bin, '2', '1', '1', '3'], capture_output=True, text=True)
    assert ok.returncode == 0 and ok.stdout.split() == ['1', '2', '0']
    past = subprocess.run([item_bin, '3', '1', '1', '3'], capture_output=True, text=True)
    assert past.returncode == -signal.SIGABRT, past
    assert 'nt > 0' in past.stderr
