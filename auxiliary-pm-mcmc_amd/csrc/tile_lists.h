// The update lists of tile_lists.cpp (entry formats: update_item.h).
#pragma once
#include <vector>

std::vector<unsigned> build_update_tiles(int i0, int R, int j0, int jend, int glo = 0, int ghi = 0);
// solo >= 0: row tile solo gets super-tile rows of its own (never paired with another row tile)
std::vector<unsigned> build_update_supertiles(int i0, int R, int j0, int jend, int glo, int ghi,
                                              int solo = -1);
std::vector<unsigned> build_update_quads(int i0, int R, int j0, int jend);
