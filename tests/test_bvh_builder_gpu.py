"""The trees the device builder (csrc/pt_bvh.hip) chooses, held against tests/bvhref.py: every case builds, downloads the traversal
copy and runs bvhref.check on every bottom level and on the top level -- membership, item order, optimality within the derived eps,
origin and exponent, boxes in both directions, slots, header facts (bvhref's docstring says what each part demands;
tests/test_bvh_builder_rules.py shows that each part notices the fault it is named for). Nothing is rendered except the two frames of
test_the_checked_tree_is_the_walked_one."""
import numpy as np
import pytest

import bvh_check
import bvhref
import isectsets as I
from test_refit import Rig, pose_of, stats_key
from test_traversal_hostile import far_small_tris, flat_grid_tris, mixed_tris

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 64, 36


# the builder's constants, restated (pt_trace.hpp blas_leaf_tris / kMaxLeafTris, pt_bvh.hip kCostTriangle / kCostInstance / kCostNode /
# kTlasCubicCells / kTlasLargeFraction, and the arguments of build_wide_tree in build_blas_device / build_tlas_device)
def leaf_rule(n):
    return 2 if n <= 32 else 1


def blas_params(n):
    return bvhref.Params(leaf_size=leaf_rule(n), max_leaf_items=3, cost_item=0.6, cubic=True, large_first=False, cost_node=1.0)


TLAS = bvhref.Params(leaf_size=1, max_leaf_items=1, cost_item=1.0, cubic=True, large_first=True, cost_node=1.0, large_fraction=0.25)

# triangles of a uniform soup in one bottom level -> what that size exercises (k_refit and k_karras run 256 leaves per workgroup)
SIZES = {
    3: "two leaves of the two-per-leaf rule, the second half full",
    31: "two per leaf with an odd last leaf",
    32: "the last size with two per leaf",
    33: "the first size with one triangle per leaf",
    70: "more than eight leaves under some child of the root: a second wide level",
    600: "three k_refit workgroups: boxes and cost tables handed from one to another",
    4096: "the last tree one workgroup collapses (kSingleGroupCollapseLeaves)",
    4097: "the first tree collapsed by one launch per level; the same checks as 4096",
    20000: "79 k_refit workgroups on the sc1 hand-off, a dozen level launches",
}
# geometry kinds, each at about 600 and about 4097 triangles
KINDS = {
    "flat_grid": "one zero extent (2e-30 after padding): cubic cells, zero-area boxes ('ties go to more roots'), exponents near -107 on y",
    "far_small": "exponents far from the coordinates' own; padding of many quanta",
    "mixed": "one huge triangle among tiny ones",
    "identical": "every key equal: the positional tree, a stable sort, all costs tied",
    "degenerate": "a soup with 10 % zero-area triangles (points and segments)",
}


def soup_tris(n, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * (0.4 / n ** (1 / 3))).astype(f32)


def kind_tris(kind, n):
    rng = np.random.default_rng(n)
    if kind == "flat_grid":
        return flat_grid_tris(n=int(np.sqrt(n / 2)) + (n > 4096))          # 17 x 17 x 2 = 578, 46 x 46 x 2 = 4232
    if kind == "far_small":
        return far_small_tris(rng, n)
    if kind == "mixed":
        return mixed_tris(rng, n - 1)
    if kind == "identical":
        return np.tile(np.array([[(0.25, 0.5, 1.0), (1.25, 0.5, 1.5), (0.5, 1.5, 1.25)]], f32), (n, 1, 1))
    t = soup_tris(n, 7)
    flat = rng.random(n) < 0.1
    seg, point = flat & (np.arange(n) % 2 == 1), flat & (np.arange(n) % 2 == 0)
    t[seg, 2] = t[seg, 1]                                     # a segment
    t[point, 1] = t[point, 0]; t[point, 2] = t[point, 0]      # a point
    return t


def build_and_check(gpu, ptamd, scene, what, parts="abcdefg"):
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    try:
        lay, buf = gpu.download_blob()
        bvh_check.check_blob(lay, buf, leaf_rule)
        res = bvhref.check(lay, buf, blas_params, TLAS, parts=parts, accel=gpu.accel_stats())
    finally:
        g.close()
    worst = max([r for _, r, _ in res["trees"].values()] + [res["tlas"][1]], key=lambda r: r["ratio"])
    print(f"[builder] {what}: cost / optimum - 1 = {worst['ratio']:.3e} (eps {worst['eps']:.3e}, H = {worst['height']}), {res['large']} large instances")
    return lay, buf, res


def single(pkg, oracle, tris):
    return I.Soup(pkg, oracle, [[tris]], [(0, I.identity())])


@pytest.mark.parametrize("n", list(SIZES))
def test_bottom_level_sizes(gpu, ptamd, pkg, oracle, n):
    tris = soup_tris(n)
    lay, buf, res = build_and_check(gpu, ptamd, single(pkg, oracle, tris).scene, f"soup {n}")
    (T, r, _), = res["trees"].values()
    assert T.n == n and T.nleaves == -(-n // leaf_rule(n))
    if n >= 70:
        assert r["depth"] >= 2
    if n >= 600:
        assert T.nleaves > 2 * 256


@pytest.mark.parametrize("n", [600, 4097])
@pytest.mark.parametrize("kind", list(KINDS))
def test_bottom_level_kinds(gpu, ptamd, pkg, oracle, kind, n):
    tris = kind_tris(kind, n)
    assert abs(len(tris) - n) <= 0.05 * n and (n < 4097 or len(tris) > 4096)
    lay, buf, res = build_and_check(gpu, ptamd, single(pkg, oracle, tris).scene, f"{kind} {len(tris)}")
    (T, r, _), = res["trees"].values()
    if kind == "identical":
        assert len(set(T.keys.tolist())) == 1 and r["optimum"] > 0


def small_instances(pkg, oracle, n, seed=21):
    rng = np.random.default_rng(seed)
    mesh = I.icosphere(pkg, 1)
    objects = [(0, I.affine(rng.uniform(0.05, 0.3, 3), rng.uniform(-4, 4, 3), rng.uniform(0, 6), rng.uniform(-1, 1))) for _ in range(n)]
    return I.Soup(pkg, oracle, [[mesh]], objects)


@pytest.mark.parametrize("n", [1, 2, 9, 300])
def test_top_level_sizes(gpu, ptamd, pkg, oracle, n):
    """1: a single leaf, no node; 2: one node of two slots; 9: more than eight, a second level; 300: two k_refit workgroups"""
    lay, buf, res = build_and_check(gpu, ptamd, small_instances(pkg, oracle, n).scene, f"top level {n}")
    assert res["tlas"][0].n == n


def test_top_level_past_the_single_workgroup_collapse(gpu, ptamd, pkg):
    """64 x 64 instances + ground + light = 4098 leaves: the top level takes the level-by-level collapse. The ground spans the scene:
    the large bit (the light, a fifth of it, stays among the small ones)."""
    scene = pkg.scenes.instanced_grid(n=64, aspect=W / H, subdiv=1)
    lay, buf, res = build_and_check(gpu, ptamd, scene, "instanced_grid 64")
    T = res["tlas"][0]
    assert T.n == 4098 > 4096 and T.large[-2] and res["large"] == 1


def test_large_instances_are_filed_apart(gpu, ptamd, pkg, oracle):
    """small instances, a ground plane under them and a box around them: the restated keys carry bit 62 for exactly those two, and the
    device's tree is the tree of those keys (membership)"""
    rng = np.random.default_rng(22)
    quad = np.array([[(-1, 0, -1), (-1, 0, 1), (1, 0, 1)], [(-1, 0, -1), (1, 0, 1), (1, 0, -1)]], f32)
    cube = np.concatenate([np.roll(np.concatenate([quad + f32((0, s, 0)) for s in (-1, 1)]), k, axis=2) for k in range(3)]).astype(f32)
    objects = [(0, I.affine(rng.uniform(0.05, 0.2, 3), rng.uniform(-4, 4, 3) * (1, 0.1, 1), rng.uniform(0, 6))) for _ in range(60)]
    objects = objects[:30] + [(1, I.affine((5, 1, 5), (0, -0.5, 0)))] + objects[30:] + [(2, I.affine((6, 6, 6)))]
    soup = I.Soup(pkg, oracle, [[I.tetrahedron()], [quad], [cube]], objects)
    lay, buf, res = build_and_check(gpu, ptamd, soup.scene, "ground and enclosure")
    T = res["tlas"][0]
    assert res["large"] == 2 and np.nonzero(T.large)[0].tolist() == [30, 61]
    assert (T.keys[T.large] >> np.uint64(62) == 1).all() and (T.keys[~T.large] >> np.uint64(62) == 0).all()


def test_an_instance_of_an_empty_mesh(gpu, ptamd, pkg, oracle):
    """an inverted instance box has a NaN centre: cell 0 on every axis, no large bit, no part in the scene bounds"""
    soup = I.Soup(pkg, oracle, [[I.tetrahedron()], [np.zeros((0, 3, 3), f32)]], [(0, I.identity()), (1, I.identity()), (0, I.affine((1, 1, 1), (3, 0, 0)))])
    lay, buf, res = build_and_check(gpu, ptamd, soup.scene, "empty mesh")
    T = res["tlas"][0]
    assert not (T.item_lo[1] <= T.item_hi[1]).any() and int(T.keys[1]) == 0


@pytest.mark.parametrize("n", [4097, 20000])
def test_the_same_input_gives_the_same_tree(gpu, ptamd, pkg, oracle, n):
    """built twice: allocation order (childBase, triBase) may differ between runs of the level-by-level collapse, the tree may not"""
    scene = single(pkg, oracle, soup_tris(n)).scene
    got = []
    for _ in range(2):
        gpu.set_sharding(0, 1, 16)
        g = ptamd.Scene(gpu, scene)
        try:
            lay, buf = gpu.download_blob()
            got.append(bvh_check.canonical_blas(lay, buf, 0, leaf_rule))
        finally:
            g.close()
    bvh_check.assert_records_equal(got[0][0], got[1][0], "nodes")
    bvh_check.assert_records_equal(got[0][1], got[1][1], "packets")


@pytest.mark.parametrize("n", [264, 4164])
def test_updatable_bottom_levels_and_refit(gpu, ptamd, oracle, pkg, n):
    """264: two k_refit workgroups; 4164: slotRefs written by the level-by-level collapse (the sizes tests/test_refit.py argues for).
    After the build every part. After a refit to the `scale` pose and back to `rest`: membership, order, slots and header facts against the
    BUILD-TIME order and tree (topology is kept), origin, exponents and boxes against the vertices as they are on the device now;
    optimality is not asked of a refitted tree."""
    rig = Rig(gpu, ptamd, oracle, pkg, (n,))
    try:
        lay, buf = gpu.download_blob()
        built = bvhref.check(lay, buf, blas_params, TLAS, accel=gpu.accel_stats())
        stats = stats_key(gpu.accel_stats())
        for kind in ("scale", "rest"):
            rig.pose(pose_of(kind, 77))
            lay, buf = gpu.download_blob()
            bvh_check.check_blob(lay, buf, leaf_rule)
            bvhref.check(lay, buf, blas_params, TLAS, parts="abdefg", accel=gpu.accel_stats(), built=built)
            assert stats_key(gpu.accel_stats())[:4] == stats[:4]
    finally:
        rig.close()


@pytest.mark.parametrize("n", [4096, 4097])
def test_the_checked_tree_is_the_walked_one(gpu, ptamd, pkg, oracle, n):
    """one frame per collapse path under PT_DEBUG_BRUTE_FORCE: the walk over the tree that was checked finds what brute force finds"""
    S = pkg.scenes
    soup = single(pkg, oracle, soup_tris(n))
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, soup.scene)
    try:
        lay, buf = gpu.download_blob()
        bvhref.check(lay, buf, blas_params, TLAS, accel=gpu.accel_stats())
        r = ptamd.Renderer(gpu, g, W, H, with_f32=True)
        gpu.set_debug_flags(2); gpu.reset_counters()
        try:
            r.render(S.graphics_settings(W, H, spp=2, bounces=4)); gpu.sync()
        finally:
            gpu.set_debug_flags(0)
        c = gpu.counters()
        assert c.SecondaryRays > 0 and c.BvhMismatches == 0 and c.StackOverflows == 0
    finally:
        g.close()
