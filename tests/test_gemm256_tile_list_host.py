"""Host: the persistent 256-tile kernels' workgroup -> tile partition (ldt_amd/csrc/gemm256_tile.h, Tile256List) against an independent
enumeration, and the dispatch rule's tiles_per_wg / one-tile family against that enumeration.  ldt_gemm_route launches nothing: no GPU.

The partition: tile ids 0 .. tiles-1 are cut into nx = min(G, 8) contiguous chunks [tiles x / nx, tiles (x + 1) / nx); the workgroups
b = x, x + nx, x + 2 nx, ... < G of label x take their chunk's ids round-robin (workgroup number j of the label: ids lo + j, lo + j + w, ...
with w = the label's workgroup count).  The one-tile kernels compute a workgroup's FIRST tile only, so they may run exactly where no
workgroup owns a second one."""
import pytest


def partition(tiles, G):
    """-> per workgroup, the list of tile ids it computes (written from the description above, not from the C++ arithmetic)"""
    nx = min(G, 8)
    out = [None] * G
    for x in range(nx):
        members = list(range(x, G, nx))
        chunk = list(range(tiles * x // nx, tiles * (x + 1) // nx))
        for j, b in enumerate(members):
            out[b] = chunk[j::len(members)]
    return out


GRIDS = (1, 3, 8, 9, 128, 164, 256)


@pytest.mark.parametrize("G", GRIDS)
def test_partition_covers_every_tile_exactly_once(G):
    for tiles in range(1, 601):
        ids = sorted(i for wg in partition(tiles, G) for i in wg)
        assert ids == list(range(tiles)), (G, tiles)


def test_grid_equal_to_tiles_is_not_one_tile_per_workgroup():
    """The case the routing correction is for: with G == tiles some workgroup owns two tiles for every count above 8 that is no multiple of 8."""
    two = [t for t in range(1, 257) if max(map(len, partition(t, t))) > 1]
    assert two == [t for t in range(9, 257) if t % 8] and len(two) == 217
    assert max(map(len, partition(164, 164))) == 2 and max(map(len, partition(9, 9))) == 2       # batch 41 x N 1024; 768 x 768


@pytest.mark.parametrize("max_wgs", [0, 128])
def test_route_reports_the_partitions_maximum(max_wgs):
    import __graft_entry__ as g
    g.build()
    from ldt_amd import ops
    lim = max_wgs or 256
    for tn in (1, 3, 4):
        for tm in range(1, 65):
            tiles = tm * tn
            G = min(tiles, lim)
            most = max(map(len, partition(tiles, G)))
            r = ops.gemm_route(ops.EPI_RESID_F32, tm * 256, tn * 256, 256, fold=256, max_wgs=max_wgs)
            assert r.family in ("256-one-tile", "256-multi-tile") and (r.bm, r.bn) == (256, 256), (tm, tn, r)
            assert r.tiles_per_wg == most, (tm, tn, max_wgs, r, most)
            assert (r.family == "256-one-tile") == (most == 1), (tm, tn, max_wgs, r, most)
