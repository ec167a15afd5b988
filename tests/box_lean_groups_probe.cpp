// Host program for tests/test_box_lean_groups.py: prints nt_box_tile_geom(width, row_count, nframes, overlapped) -- the block
// shape box_tile_kernel is launched with -- for each (width, row_count, nframes, overlapped) quadruple given on the command
// line, one "rows waves" line per quadruple.  (tests/box_tile_geom_probe.cpp is the same without `overlapped`.)
#include <stdio.h>
#include <stdlib.h>

#include "nt_device.hpp"

int main(int argc, char **argv) {
    if (argc < 5 || (argc - 1) % 4 != 0) {
        fprintf(stderr, "usage: %s width row_count nframes overlapped [...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 3 < argc; i += 4) {
        const NtBoxTileGeom g = nt_box_tile_geom(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]));
        printf("%d %d\n", g.rows, g.waves);
    }
    return 0;
}
