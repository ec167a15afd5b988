// Host program for tests/test_box_tile_shapes.py: prints nt_box_tile_geom(width, row_count, nframes, 0) -- the block shape
// box_tile_kernel is launched with -- for each (width, row_count, nframes) triple given on the command line, one
// "rows waves" line per triple.  nt_device.hpp is host-compilable on its own (g++ -std=c++17 -I ntracer_amd/csrc).
#include <stdio.h>
#include <stdlib.h>

#include "nt_device.hpp"

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: %s width row_count nframes [width row_count nframes ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 2 < argc; i += 3) {
        const NtBoxTileGeom g = nt_box_tile_geom(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), 0);
        printf("%d %d\n", g.rows, g.waves);
    }
    return 0;
}
