"""The update lists of csrc/tile_lists.cpp (plain C++, no GPU): every tile (i, j) with i in
[i0, R) outside the gap and j0 <= j <= min(i, jend - 1) is written by exactly one entry of each of
the three lists, and no other tile is. The file is compiled with the host compiler and a small
main into a temporary directory. The entry formats are stated twice: written() below decodes them
in Python, on its own, and the main prints the tiles that the entry structs of csrc/update_item.h
(what the builders pack with and the kernels unpack with) say each entry writes; the two agree."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'auxiliary-pm-mcmc_amd', 'csrc')

MAIN = r'''
#include <cstdio>
#include "tile_lists.h"
#include "update_item.h"
template <class Entry>
static void show(unsigned packed) {  // "entry:i.j,i.j,.. ": the tiles writes() yields
    const Entry e(packed);
    printf("%x:", packed);
    for (int a = 0; a < Entry::E; ++a)
        for (int c = 0; c < Entry::E; ++c)
            if (e.writes(a, c)) printf("%d.%d,", e.i() + a, e.j() + c);
    printf(" ");
}
int main() {  // per input line "kind i0 R j0 jend glo ghi solo": the list's entries in hex
    int k, i0, R, j0, je, glo, ghi, solo;
    while (scanf("%d %d %d %d %d %d %d %d", &k, &i0, &R, &j0, &je, &glo, &ghi, &solo) == 8) {
        const std::vector<unsigned> v =
            k == 0 ? build_update_tiles(i0, R, j0, je, glo, ghi)
                   : k == 1 ? build_update_supertiles(i0, R, j0, je, glo, ghi, solo)
                            : build_update_quads(i0, R, j0, je);
        for (unsigned e : v) k == 0 ? show<Tile64>(e) : k == 1 ? show<SuperTile>(e) : show<QuadTile>(e);
        printf("\n");
    }
    return 0;
}
'''
TILES, SUPER, QUADS = 0, 1, 2


def host_compiler():
    for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def lists_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp('tile_lists')
    src = d / 'main.cpp'
    src.write_text(MAIN)
    exe = str(d / 'tile_lists_main')
    subprocess.check_call([host_compiler(), '-std=c++17', '-O1', '-Wall', '-I', CSRC, str(src),
                           os.path.join(CSRC, 'tile_lists.cpp'), '-o', exe])
    return exe


def written(kind, entries):
    """The tiles the kernels write for a list's entries, with repeats."""
    out = []
    for e in entries:
        if kind == TILES:
            out.append((e >> 16, e & 0xffff))
        elif kind == SUPER:
            i, j = e >> 18, (e >> 4) & 0x3fff
            out += [(i + a, j + c) for a in range(2) for c in range(2)
                    if (e >> a) & 1 and (e >> (2 + c)) & 1 and j + c <= i + a]
        else:
            i, j, rm, cm = e >> 20, (e >> 8) & 0xfff, (e >> 4) & 15, e & 15
            out += [(i + a, j + c) for a in range(4) for c in range(4)
                    if (rm >> a) & 1 and (cm >> c) & 1 and j + c <= i + a]
    return out


def expected(i0, R, j0, jend, glo=0, ghi=0):
    return sorted((i, j) for i in range(i0, R) if not glo <= i < ghi
                  for j in range(j0, min(i, jend - 1) + 1))


def shapes(nb):
    """(i0, R, j0, jend) as the factorisations launch them: a panel's trailing update (i0 = j0 =
    Kend), its narrow and far parts, rows starting below the columns, with and without the
    appended right-hand-side row tile nb."""
    out = set()
    for kend in sorted({0, 1, 2, 8, nb - 1} & set(range(nb))):
        for R in (nb, nb + 1):
            for jend in sorted({kend + 1, kend + 2, min(kend + 8, nb), nb}):
                if jend <= nb:
                    out.add((kend, R, kend, jend))
                    out.add((min(jend, R - 1), R, kend, jend))  # rows below the columns' diagonal
    return sorted(out)


def check(lists_bin, cases):
    """cases: (kind, builder arguments, expected tiles); returns each case's entries"""
    text = ''.join('{0} {1}\n'.format(k, ' '.join(map(str, a))) for k, a, _ in cases)
    res = subprocess.run([lists_bin], input=text, capture_output=True, text=True, check=True)
    lines = res.stdout.split('\n')
    assert len(lines) == len(cases) + 1
    out = []
    for (kind, args, want), line in zip(cases, lines):
        entries = []
        for tok in line.split():
            e, tiles = tok.split(':')
            entries.append(int(e, 16))
            header = [tuple(map(int, t.split('.'))) for t in tiles.split(',') if t]
            assert header == written(kind, entries[-1:]), (kind, args, e)  # writes() == written()
        got = written(kind, entries)
        assert sorted(got) == want, (kind, args)  # (sorted with repeats: exactly once each)
        if kind == SUPER and args[6] >= 0:  # the solo row tile shares no entry with another row
            for e in entries:
                rows = {(e >> 18) + a for a in range(2) if (e >> a) & 1}
                assert args[6] not in rows or rows == {args[6]}, (args, hex(e))
        out.append(entries)
    return out


@pytest.mark.parametrize('nb', [1, 2, 3, 5, 9, 18])
def test_every_tile_written_exactly_once(lists_bin, nb):
    cases = []  # (kind, builder arguments, expected tiles)
    for i0, R, j0, jend in shapes(nb):
        solo = nb if R > nb else -1
        cases.append((TILES, (i0, R, j0, jend, 0, 0, -1), expected(i0, R, j0, jend)))
        cases.append((TILES, (i0, R, j0, jend, 2, 4, -1), expected(i0, R, j0, jend, 2, 4)))
        cases.append((SUPER, (i0, R, j0, jend, 0, 0, -1), expected(i0, R, j0, jend)))
        cases.append((SUPER, (i0, R, j0, jend, 0, 0, solo), expected(i0, R, j0, jend)))
        cases.append((SUPER, (i0, R, j0, jend, 2, 4, solo), expected(i0, R, j0, jend, 2, 4)))
        cases.append((QUADS, (i0, R, j0, jend, 0, 0, -1), expected(i0, R, j0, jend)))
        if R > nb and jend < nb:  # the right-hand-side row's columns beyond jend, on their own
            cases.append((SUPER, (nb, nb + 1, jend, nb, 0, 0, nb), expected(nb, nb + 1, jend, nb)))
    check(lists_bin, cases)


def test_gap_and_solo_in_one_list(lists_bin):
    """Row tiles 3 .. 5 left out and row tile 7 on its own, both inside the list. The builder
    pairs the rows from i0 on whatever the gap: (1, 2), (3, 4), (5, 6), (7), (8, 9). The pair
    (3, 4) lies in the gap and has no entry; of (5, 6) only the lower half is valid (an entry
    whose first row half is the invalid one); 7 is alone."""
    args = (1, 10, 1, 9, 3, 6, 7)
    entries, = check(lists_bin, [(SUPER, args, expected(1, 10, 1, 9, 3, 6))])
    rows = {(e >> 18, e & 3) for e in entries}  # (first row tile, rv0 | rv1 << 1)
    assert rows == {(1, 3), (5, 2), (7, 1), (8, 3)}


def test_quad_with_partial_last_row_and_column(lists_bin):
    """R = 6 and jend = 5: the second quad row holds row tiles 4 and 5 only (rmask 0b0011), the
    second quad column holds column tile 4 only (cmask 0b0001)."""
    entries, = check(lists_bin, [(QUADS, (0, 6, 0, 5, 0, 0, -1), expected(0, 6, 0, 5))])
    assert [(e >> 20, (e >> 8) & 0xfff, (e >> 4) & 15, e & 15) for e in entries] == \
        [(0, 0, 15, 15), (4, 0, 3, 15), (4, 4, 3, 1)]
