"""CPU checks of the ReGIR Onion layout (pt_di_set_regir_layout): the settings struct, the enum and the exports against the header; the
library's static tables against the float64 restatement of the spec (tests/onionref.py); the self-consistency of the lookup on those
tables; the mutations the restatement must tell apart; and what the layout is for: the floor of emitter_field at a small cell size."""
import os
import re

import numpy as np
import pytest

import onionref as O
import presamplingref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptamd.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def tables(ptamd):
    return O.Tables(*[ptamd.onion_table(w) for w in range(4)])


def test_layout_struct_enum_and_exports_match_header(pkg, ptamd):
    L = pkg.layouts
    text = _header()
    body = re.search(r"typedef struct PtDIReGIRLayoutSettings \{(.*?)\} PtDIReGIRLayoutSettings;", text, re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["uint32_t Layout", "uint32_t _pad[3]"]
    dt = L.DI_REGIR_LAYOUT_SETTINGS
    assert dt.itemsize == 16 and list(dt.names) == ["Layout", "_pad"]
    assert (dt.fields["Layout"][1], dt.fields["_pad"][1], dt.fields["_pad"][0].itemsize) == (0, 4, 12)
    enum = re.search(r"enum \{ PT_DI_REGIR_LAYOUT_GRID = (\d+), PT_DI_REGIR_LAYOUT_ONION = (\d+) \};", text)
    assert (int(enum.group(1)), int(enum.group(2))) == (L.DI_REGIR_LAYOUT_GRID, L.DI_REGIR_LAYOUT_ONION) == (0, 1)
    assert re.search(r"int\s+pt_di_set_regir_layout\(PtContext\* ctx, const PtDIReGIRLayoutSettings\* settings\);", text)
    assert re.search(r"int\s+pt_di_regir_onion_table\(uint32_t which, float\* host_dst, uint32_t capacity, uint32_t\* out_count\);", text)
    lib = ptamd.load_library()
    for sym in ("pt_di_set_regir_layout", "pt_di_regir_onion_table"):
        assert sym in ptamd.EXPORTS and hasattr(lib, sym), sym
    assert L.di_regir_layout_settings().tobytes() == bytes(16) == L.di_regir_layout_settings("grid").tobytes()
    assert L.di_regir_layout_settings("onion").tobytes() == bytes([1, 0, 0, 0]) + bytes(12)
    assert int(L.di_regir_layout_settings(2)["Layout"]) == 2
    # the light-sampling struct is the one it was
    assert L.DI_LIGHT_SAMPLING_SETTINGS.itemsize == 16 and list(L.DI_LIGHT_SAMPLING_SETTINGS.names) == ["Mode", "ReGIRCellSize", "ReGIRBuildSamples"]


def test_onion_table_call_contract(ptamd):
    import ctypes as C
    lib = ptamd.load_library()
    n = C.c_uint32(7)
    assert lib.pt_di_regir_onion_table(4, None, 0, C.byref(n)) != 0 and n.value == 7          # an unknown table: refused, nothing written
    assert lib.pt_di_regir_onion_table(0, None, 0, None) != 0
    assert lib.pt_di_regir_onion_table(0, None, 4, C.byref(n)) != 0
    part = np.full(6, -1.0, f32)
    assert lib.pt_di_regir_onion_table(3, C.c_void_p(part.ctypes.data), 4, C.byref(n)) == 0 and n.value == 4 * O.CELLS
    assert part.tolist() == [0, 0, 0, 1, -1, -1]                                                # capacity floats and no more
    with pytest.raises(ptamd.PtInvalidArgument):
        ptamd.onion_table(4)
    assert [ptamd.onion_table(w).shape for w in range(4)] == [(16,), (20,), (241,), (O.CELLS, 4)]


def test_static_structure():
    """the spec's counts: rings per group, cells per layer, 2253 cells, B_15"""
    for g, p in enumerate(O.PARTITIONS):
        assert len(O.RING_CELLS[g]) == p // 4 + 1 and O.RING_CELLS[g][0] == p and O.RING_CELLS[g][-1] == 1
    assert [O.LAYER_CELLS[l] for l in (0, 1, 2, 3, 4, 14)] == [20, 46, 80, 126, 180, 180]
    assert 1 + sum(O.LAYER_CELLS) == O.CELLS == 2253 == 1 + 20 + 46 + 80 + 126 + 11 * 180
    b2, ring, az, cells = O.tables64()
    assert (len(b2), len(ring), len(az), len(cells)) == (16, 20, 241, 2253)
    assert abs(np.sqrt(b2[15]) - 145.055) < 1e-3 and b2[0] == 1.0
    assert np.all(np.diff(b2) > 0)
    at = 0
    for g, k in O.ROWS:                                       # azimuth thresholds rise within a ring, inside (0, 4)
        n = O.RING_CELLS[g][k]
        t = az[at:at + n - 1]; at += n - 1
        assert np.all(np.diff(t) > 0) and (n == 1 or (t[0] > 0 and t[-1] < 4))
    assert tuple(cells[0]) == (0, 0, 0, 1)
    # the listed cells per ring keep the cells near square: the ring's circumference over the ring's height, to the nearest cell count
    # within one (not the rule that made them: the list is the spec)
    for g, p in enumerate(O.PARTITIONS):
        for k in range(1, p // 4):
            assert abs(O.RING_CELLS[g][k] - p * np.cos(k * 2 * np.pi / p)) <= 1.5, (g, k)


def test_library_tables_within_one_ulp_of_float64(ptamd):
    for which, ref in enumerate(O.tables64()):
        got = ptamd.onion_table(which).astype(np.float64)
        ref = np.asarray(ref, np.float64).reshape(got.shape)
        ulp = np.spacing(np.maximum(np.abs(ref), np.finfo(f32).tiny).astype(f32)).astype(np.float64)
        # a centre coordinate that is 0 up to the rounding of cos(pi / 2) * r: one ulp of the cell's own size
        if which == 3:
            ulp = np.maximum(ulp, np.spacing(ref[:, 3:4].astype(f32)).astype(np.float64) * (np.abs(ref) < 1e-9))
        err = np.abs(got - ref) / ulp
        assert err.max() <= 1.0, (which, err.max(), int(err.argmax()))


@pytest.mark.parametrize("c", [0.05, 0.37, 5.0])
def test_every_cell_centre_looks_up_to_its_own_index(tables, c):
    v = (f32(c) * tables.cells[:, :3]).astype(f32)
    assert np.array_equal(O.lookup(tables, v, c), np.arange(O.CELLS))


def _random_points(rng, n, reach):
    """points spread over the layers (log-uniform radius) and uniformly over directions"""
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.exp(rng.uniform(np.log(0.05), np.log(reach), n))
    return (d * r[:, None]).astype(f32)


def test_random_points_lie_in_their_cells_sphere(tables):
    rng = np.random.default_rng(5)
    c = 0.37
    reach = float(np.sqrt(np.float64(tables.b2[15]))) * c * 0.999
    v = _random_points(rng, 20000, reach)
    cell = O.lookup(tables, v, c)
    assert (cell >= 0).all() and len(np.unique(cell)) > 1500
    centre, radius = O.cell_spheres(tables, cell, np.zeros(3, f32), 2 * c)
    ratio = np.linalg.norm(v.astype(np.float64) - centre, axis=1) / radius
    print(f"largest distance / radius: {ratio.max():.4f}")
    assert ratio.max() <= 1.0


def test_edges_of_the_lookup(tables):
    c = f32(0.37)
    reach = np.sqrt(np.float64(tables.b2[15])) * float(c)
    out = np.array([[reach * 1.0001, 0, 0], [0, -reach * 1.0001, 0], [1e9, 1e9, 1e9], [np.inf, 0, 0], [np.nan, 0, 0]], f32)
    assert (O.lookup(tables, out, c) == -1).all()
    inner = np.array([[0, 0, 0], [0.36, 0, 0], [0, -0.2, 0.2], [-0.0, 0.0, -0.0]], f32)
    assert (O.lookup(tables, inner, c) == 0).all()
    # q = 1 exactly is the first layer, q just below b2[15] the last
    assert O.lookup(tables, np.array([[c, 0, 0]], f32), c)[0] == O.LAYER_BASE[0]
    last = O.lookup(tables, np.array([[reach * 0.9999, 0, 0]], f32), c)[0]
    assert O.LAYER_BASE[14] <= last < O.CELLS
    # the poles (x = z = 0) are the layers' caps, north the last but one cell of the layer and south the last; signed zeros change nothing
    for layer in range(O.LAYERS):
        r = float(c) * 0.5 * (np.sqrt(np.float64(tables.b2[layer])) + np.sqrt(np.float64(tables.b2[layer + 1])))
        end = O.LAYER_BASE[layer] + O.LAYER_CELLS[layer]
        got = O.lookup(tables, np.array([[0, r, 0], [0, -r, 0], [-0.0, r, -0.0], [0.0, -r, -0.0]], f32), c)
        assert got.tolist() == [end - 2, end - 1, end - 2, end - 1], layer
    # y = 0: ring 0 whatever the sign of the zero, every azimuth cell of it in order; the azimuth starts at +x and turns towards +z
    for layer in (0, 3, 9):
        n = O.RING_CELLS[O.LAYER_GROUP[layer]][0]
        r = float(c) * 0.5 * (np.sqrt(np.float64(tables.b2[layer])) + np.sqrt(np.float64(tables.b2[layer + 1])))
        a = (np.arange(n) + 0.5) * 2 * np.pi / n
        for y in (0.0, -0.0):
            v = np.stack([r * np.cos(a), np.full(n, y), r * np.sin(a)], -1).astype(f32)
            assert np.array_equal(O.lookup(tables, v, c), O.LAYER_BASE[layer] + np.arange(n))
    # the diamond angle is monotone in the true angle and stays in [0, 4)
    a = np.linspace(0, 2 * np.pi, 4001)[:-1]
    A = O.diamond32(np.cos(a).astype(f32), np.sin(a).astype(f32))
    assert np.all(np.diff(A.astype(np.float64)) > 0) and A[0] == 0 and A[-1] < 4
    assert O.diamond32(f32(0), f32(0)) == 0 and O.diamond32(f32(-0.0), f32(-0.0)) == 0


def test_mutations_are_told_apart(tables):
    """south before north, c without the 0.5, the jitter without its distance term, an azimuth count from j = 0: each changes what the
    restatement returns, on the inputs the other tests use"""
    c = 0.37
    v = (f32(c) * tables.cells[:, :3]).astype(f32)
    own = np.arange(O.CELLS)
    assert np.array_equal(O.lookup(tables, v, c), own)
    south = O.lookup(tables, v, c, south_first=True)
    two_hemispheres = np.abs(tables.cells[:, 1]) > 1e-3 * tables.cells[:, 3]                  # every ring but ring 0
    assert (south != own)[two_hemispheres].all() and (south == own)[~two_hemispheres].all()
    az0 = O.lookup(tables, v, c, azimuth_from_zero=True)
    assert (az0[1:] != own[1:]).all()
    rng = np.random.default_rng(9)
    centre = np.array([0.3, 2.0, -3.5], f32)
    Pw = centre + _random_points(rng, 4000, 20.0)
    draws = rng.random((4000, 3)).astype(f32)
    ref = O.onion_cell(tables, Pw, draws, centre, 2 * c)
    assert (ref >= 0).all()
    full = O.onion_cell(tables, Pw, draws, centre, 2 * c, half=False)
    assert (full != ref).mean() > 0.5
    flat = O.onion_cell(tables, Pw, draws, centre, 2 * c, distance_term=False)
    far = np.linalg.norm(Pw - centre, axis=1) > 10 * c
    assert (flat != ref)[far].mean() > 0.2
    # and the jitter does what it is for: it moves a point by at most one scale per axis, the scale the larger of c and pi / 12 of the distance
    v, cc = O.jittered(Pw, draws, centre, 2 * c)
    d = np.linalg.norm(Pw - centre, axis=1)
    assert cc == f32(c) and np.all(np.abs(v - (Pw - centre)).max(1) <= np.maximum(c, 0.2617994 * d) * (1 + 1e-6))
    v1, _ = O.jittered(Pw, np.full_like(draws, 0.5), centre, 2 * c)
    assert np.array_equal(v1, (Pw - centre).astype(f32))


def test_coverage_of_the_emitter_field_floor(pkg, tables):
    """5000 points of emitter_field's floor at ReGIRCellSize 0.3: most lie outside the 16^3 grid (which falls back to Power_RIS there),
    none outside the onion, jittered or not"""
    scene = pkg.scenes.emitter_field(16)
    centre = scene.camera["Position"].astype(f32).reshape(3)
    rng = np.random.default_rng(2)
    Pw = np.stack([rng.uniform(-8, 8, 5000), np.zeros(5000), rng.uniform(-8, 8, 5000)], -1).astype(f32)
    draws = rng.random((5000, 3)).astype(f32)
    grid = P.regir_cell(Pw, draws, centre, 0.3)
    onion = O.onion_cell(tables, Pw, draws, centre, 0.3)
    print(f"outside the grid: {(grid < 0).mean():.3f}; outside the onion: {(onion < 0).mean():.3f}; onion reach "
          f"{0.15 * np.sqrt(np.float64(tables.b2[15])):.1f}")
    assert (grid < 0).mean() > 0.5
    assert (onion >= 0).all() and (O.lookup(tables, Pw - centre, 0.15) >= 0).all()
