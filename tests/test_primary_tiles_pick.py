"""Which build of the level-1 kernel serves a request, and the grid it is launched with (csrc/p3d_kernel_variant.h),
compiled for the host: several tiles per workgroup exist for LDS scenes on the per-lane walk without counters, features
or batches, every other request runs one tile per workgroup, and the 2-D grid covers every tile row of a band exactly
once whatever the remainder (CPU only)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO

SRC = r"""
#include "p3d_kernel_variant.h"
using namespace p3d;
static KernelVariant request(int count, int lds, int walk, int occ, int stoch, int schlick, int batch, int tiles) {
    KernelVariant v;
    v.count = count; v.lds = lds; v.walk = walk; v.occ = occ; v.stoch = stoch; v.schlick = schlick; v.batch = batch; v.tiles = tiles;
    return v;
}
extern "C" {
// tiles of the build that serves the request as level kernel k (0 primary, 1 secondary, 2 tile); -1: that build does not exist
int served_tiles(int k, int count, int lds, int walk, int occ, int stoch, int schlick, int batch, int tiles) {
    const KernelVariant s = canonical_level(request(count, lds, walk, occ, stoch, schlick, batch, tiles), (Level)k);
    return built_level(s, (Level)k) ? s.tiles : -1;
}
int served_occ(int occ, int tiles) { return canonical_level(request(0, 1, WALK_LANE, occ, 0, 0, 0, tiles), Level::Primary).occ; }
// the level-1 launch of a plain LDS request over a band: tiles | grid.x << 8 | grid.y << 20
int launch(int lds, int tiles, int tiles_x, int tile_rows, int xcd_chunk, int grid_blocks) {
    const KernelVariant s = served_primary(request(0, lds, lds ? WALK_LANE : WALK_SHARED, 6, 0, 0, 0, tiles), tiles_x, tile_rows, tiles_x * tile_rows, xcd_chunk);
    const PrimaryGrid g = primary_grid(s, tiles_x, tile_rows, tiles_x * tile_rows, xcd_chunk, grid_blocks);
    return s.tiles | (int)g.x << 8 | (int)g.y << 20;
}
int max_tiles() { return kMaxPrimaryTiles; }
int default_tiles() { return kDefaultPrimaryTiles; }
}
"""
PRIMARY, SECONDARY, TILE = 0, 1, 2
LANE, PACKET, GRID, SHARED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiles")
    (d / "tiles.cpp").write_text(SRC)
    inc = ["-I" + os.path.join(REPO, "u_4a_2s_p3d_raytracer_template2_amd", "csrc")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC"] + inc + [str(d / "tiles.cpp"), "-o", str(d / "tiles.so")])
    return C.CDLL(str(d / "tiles.so"))


def test_only_the_plain_lds_level1_builds_have_several_tiles(lib):
    assert lib.max_tiles() == 3 and 1 <= lib.default_tiles() <= 3
    for t in (1, 2, 3):
        for occ in (0, 1, 5, 6):
            assert lib.served_tiles(PRIMARY, 0, 1, LANE, occ, 0, 0, 0, t) == t
        assert lib.served_tiles(PRIMARY, 0, 1, SHARED, 6, 0, 0, 0, t) == t          # LDS scenes have no shared walk: served by the lane walk
    assert lib.served_occ(6, 3) == 6 and lib.served_occ(5, 2) == 5 and lib.served_occ(8, 2) == 1
    for t in (2, 3):
        assert lib.served_tiles(PRIMARY, 1, 1, LANE, 6, 0, 0, 0, t) == 1             # counting build
        assert lib.served_tiles(PRIMARY, 0, 0, LANE, 6, 0, 0, 0, t) == 1             # scene read from HBM
        assert lib.served_tiles(PRIMARY, 0, 0, SHARED, 6, 0, 0, 0, t) == 1
        assert lib.served_tiles(PRIMARY, 0, 1, PACKET, 6, 0, 0, 0, t) == 1
        assert lib.served_tiles(PRIMARY, 0, 1, GRID, 6, 0, 0, 0, t) == 1
        assert lib.served_tiles(PRIMARY, 0, 1, LANE, 6, 1, 0, 0, t) == 1             # features with random draws
        assert lib.served_tiles(PRIMARY, 0, 1, LANE, 6, 0, 1, 0, t) == 1             # Schlick
        assert lib.served_tiles(PRIMARY, 0, 1, LANE, 6, 0, 0, 1, t) == 1             # frame batch
        assert lib.served_tiles(SECONDARY, 0, 1, LANE, 6, 0, 0, 0, t) == 1           # the other level kernels have no such variant
        assert lib.served_tiles(TILE, 0, 1, LANE, 6, 0, 0, 0, t) == 1
    for t in (-1, 0, 4, 64):                                                         # out of range: one tile, never a missing build
        assert lib.served_tiles(PRIMARY, 0, 1, LANE, 6, 0, 0, 0, t) == 1


def test_every_request_reaches_a_build(lib):
    for k in (PRIMARY, SECONDARY, TILE):
        for bits in range(64):
            count, lds, stoch, schlick, batch = [(bits >> i) & 1 for i in range(5)]
            for walk in (LANE, PACKET, GRID, SHARED):
                for occ in (0, 5, 6):
                    for t in (1, 2, 3):
                        assert lib.served_tiles(k, count, lds, walk, occ, stoch, schlick, batch, t) >= 1


# (res_x, local rows) of the GPU test's frames: one tile; three tile rows with a ragged right edge; seven tile rows; rank 1
# of 3 with row_block 16 on 64x112 (its row blocks 1 and 4: two tile rows); and the headline frame
BANDS = [(16, 16), (50, 36), (64, 112), (64, 32), (1920, 1080)]


@pytest.mark.parametrize("res_x,rows", BANDS)
@pytest.mark.parametrize("tiles", [1, 2, 3])
def test_the_grid_covers_every_tile_row_once(lib, res_x, rows, tiles):
    tiles_x, tile_rows = (res_x + 15) // 16, (rows + 15) // 16
    r = lib.launch(1, tiles, tiles_x, tile_rows, 1, 8 * ((tiles_x * tile_rows + 7) // 8))
    t, gx, gy = r & 255, (r >> 8) & 4095, r >> 20
    if tiles == 1 and tile_rows == 1:
        assert (t, gy) == (1, 1) and gx >= tiles_x          # one tile row: the 1-D launch, as before
        return
    assert t == tiles and gx == tiles_x and gy == -(-tile_rows // tiles)
    seen = sorted(by + k * gy for by in range(gy) for k in range(t) if by + k * gy < tile_rows)      # the kernel's loop
    assert seen == list(range(tile_rows))
    assert gy * t - tile_rows < t                            # fewer empty iterations than one workgroup's share


def test_no_2d_launch_no_tiles(lib):
    # a chunked tile map (xcd_chunk > 1) and scenes read from HBM number their tiles 1-D: one tile per workgroup
    for tiles in (2, 3):
        assert lib.launch(1, tiles, 4, 7, 2, 32) == 1 | 32 << 8 | 1 << 20
        assert lib.launch(0, tiles, 4, 7, 1, 32) == 1 | 32 << 8 | 1 << 20
