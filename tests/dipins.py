"""What the per-pixel direct-lighting pins share when they run at frame sizes that do not fill a tile.

The DI kernels lay a frame out in 16 x 16 blocks of four 8 x 8 wave tiles (the boiling filter's 64-lane butterfly sums one such tile),
Power_RIS and ReGIR pick a light tile per 16 x 16 screen tile, and the reuse passes reflect neighbour and history positions at the view's
edges and turn pixel indices back into (x, y) with the frame's width. The pins' own sizes (48 x 32, 40 x 24, 80 x 60) are multiples of 8
at least; the sizes here cut every one of those tiles on both axes, with an odd width and an odd height.

A ragged run must also show that it reached the edges: assert_edge_witnesses reads the counters the reference modules keep
(restirref.note) while they restate a frame."""

# 37 x 23: 851 pixels, 3 x 2 blocks, 5 x 3 wave tiles, 3 x 2 screen tiles, the last of each cut on both axes.
# 21 x 13: 273 pixels, 2 x 1 blocks, 3 x 2 wave tiles, every block cut.
RAGGED = [(37, 23), (21, 13)]


def size_id(size):
    return f"{size[0]}x{size[1]}"


def more_than(value, count, W, H, W0, H0):
    """`value > count`, where a pin states the coverage floor `count` for its W0 x H0 frame ("more than 20 occluded pixels"), taken as
    the same share of a W x H frame: the floor says that the frame shows a thing at all, so it scales with the pixels there are. At
    W0 x H0 it is `value > count` itself."""
    return value * W0 * H0 > count * W * H


def assert_edge_witnesses(stats, W, H, what, temporal=False, spatial=False, boiling=False):
    """stats: what restirref / pairwiseref counted over the frames of one ragged run. A spatial pass must have reflected a neighbour at the
    right edge and one at the bottom edge; a temporal pass must have had a search position reflected, or rejected outside the view; a
    boiling filter must have decided in a tile that the frame's edge cuts, over a nonzero count of reservoirs."""
    assert W % 8 and H % 8, "a ragged size cuts the 8 x 8 wave tile on both axes"
    keys = sorted(k for k in stats if k.split("_")[0] in ("spatial", "temporal", "boiling"))
    print(f"{what} at {W} x {H}: edge witnesses " + ", ".join(f"{k} {stats[k]}" for k in keys))
    if spatial:
        assert stats.get("spatial_right", 0) > 0 and stats.get("spatial_bottom", 0) > 0, (what, stats)
    if temporal:
        met = sum(stats.get("temporal_" + k, 0) for k in ("left", "top", "right", "bottom", "outside"))
        assert met > 0, (what, stats)
    if boiling:
        assert stats.get("boiling_cut_tiles", 0) > 0 and stats.get("boiling_cut_count", 0) > 0, (what, stats)
