"""The box test and the builders on scenes that are neither unit-scale nor origin-centred.

wide_node_hits moves every slab plane outward by (|b| + 255 |a|) * 2^-21 and the builders quantise child boxes to 8 bits against the node
origin: both are scale-dependent arguments, and every traversal scene so far sat around the origin at a size of one. A box test that is not
conservative drops hits silently, so here the walk is held against brute force (no box test at all) ray by ray, bit for bit:

  far_small   1 200 triangles of size 1e-2 around (4096.5, -2048.25, 1024.125)
  flat_grid   an axis-aligned grid in the plane y = 0: zero-thickness child boxes; rays in the plane, along the axes, and from origins
              exactly on node-box planes (decoded from the downloaded blob by bvh_check)
  mixed       1 000 slivers of size 1e-3 next to one triangle of size 1e3, in one bottom level
  instanced   far_small and mixed as instances under 1e-3, 1e3, mirrored and sheared-scale transforms

Per scene 20 000 rays (random ones, and rays aimed at vertices, edge points and interiors from every distance) through
pt_debug_trace_closest with and without PT_DEBUG_BRUTE_FORCE: identical records, no refused push, and equal to the oracle's brute force.
One 64x48 frame per schedule (default, _PHASED, _V1, _UNFUSED_ROUNDS) equals the oracle's brute-force frame, PT_DEBUG_BRUTE_FORCE counts no
mismatch, bvh_check.check_blob passes. On the CPU the oracle's own BVH is held against its brute force on the same rays, and a sample of
the records against the exact closest hit (tests/isectref.py)."""
import functools

import numpy as np
import pytest

import bvh_check
import isectref as R
import isectsets as I

f32, f64 = np.float32, np.float64
W, H = 64, 48
FAR = np.array([4096.5, -2048.25, 1024.125])
RAYS = 20000
SCENES = ("far_small", "flat_grid", "mixed", "instanced")


def far_small_tris(rng, n=1200):
    c = FAR + rng.uniform(-0.25, 0.25, (n, 1, 3))
    return (c + rng.normal(size=(n, 3, 3)) * 1e-2).astype(f32)


def flat_grid_tris(n=24, half=3.0):
    xs = np.linspace(-half, half, n + 1)
    tris = []
    for j in range(n):
        for i in range(n):
            p = [(xs[i], 0, xs[j]), (xs[i + 1], 0, xs[j]), (xs[i + 1], 0, xs[j + 1]), (xs[i], 0, xs[j + 1])]
            tris += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    return np.array(tris, f32)


def mixed_tris(rng, n=1000):
    big = np.array([[(-500, 0, -300), (500, 0, -300), (0, 0, 700)]], f64)
    c = rng.uniform(-0.05, 0.05, (n, 1, 3)); c[:, :, 1] = rng.uniform(0.001, 0.05, (n, 1))
    along = rng.normal(size=(n, 1, 3)); along /= np.linalg.norm(along, axis=-1, keepdims=True)
    s = np.array([-0.5, 0.5, 0.0]).reshape(1, 3, 1) * 1e-3 * along + rng.normal(size=(n, 3, 3)) * 2e-5       # long and thin
    return np.concatenate([big, c + s]).astype(f32)


@functools.lru_cache(None)
def hostile(name):
    """(Soup, rays [RAYS, 8])"""
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L
    import dxpbrt_amd.scenes as S

    class P:
        layouts, scenes = L, S
    oracle = ge.load_oracle()
    rng = np.random.default_rng({"far_small": 11, "flat_grid": 12, "mixed": 13, "instanced": 14}[name])
    cam = lambda pos, fwd, fov=70.0: S.make_camera(pos, forward=fwd, hfov_deg=fov, aspect=W / H)
    if name == "far_small":
        soup = I.Soup(P, oracle, [[far_small_tris(rng)]], [(0, I.identity())], cam(FAR + (0, 0, -0.7), (0, 0, 1)))
    elif name == "flat_grid":
        soup = I.Soup(P, oracle, [[flat_grid_tris()]], [(0, I.identity())], cam((0.1, 1.5, -4.0), (0, -0.35, 1)))
    elif name == "mixed":
        soup = I.Soup(P, oracle, [[mixed_tris(rng)]], [(0, I.identity())], cam((0, 0.05, -0.15), (0, -0.2, 1)))
    else:
        a, c = far_small_tris(np.random.default_rng(11), 700), mixed_tris(np.random.default_rng(13), 700)
        up = I.affine((1e3,) * 3, (0, 0, 0), 0.3, 0.1); up[:, 3] = (np.array([0, 0, 900.0]) - up[:, :3].astype(f64) @ FAR).astype(f32)     # lands around (0, 0, 900)
        down = I.affine((1e-3,) * 3, (0, 0, 0), -0.5, 0.2); down[:, 3] = (np.array([0.2, 0.1, 1.0]) - down[:, :3].astype(f64) @ FAR).astype(f32)
        objects = [(0, up), (0, down), (1, I.affine((-1, 1, 1), (0.3, -0.2, 2.0), 0.8, -0.3)), (1, I.affine((1e-3,) * 3, (-0.2, 0.3, 1.5), 1.0, 0.5)),
                   (1, I.affine((1e3, 1e3, 1e3), (100.0, -2000.0, 300.0), 0.2, 0.0)), (1, I.affine((1.0, -1.5, 0.5), (0.0, 0.4, 2.5), 2.0, 1.0))]
        soup = I.Soup(P, oracle, [[a], [c]], objects, cam((0, 0.5, -3.0), (0, -0.05, 1)))
    return soup, hostile_rays(soup, rng)


def world_triangles(soup):
    out = []
    for (n, m), (w2o, tris, geom, prim) in zip(soup.objects, soup.instances):
        out.append(tris.astype(f64) @ m[:, :3].astype(f64).T + m[:, 3].astype(f64))
    return out


def hostile_rays(soup, rng, count=RAYS):
    """Half aimed -- at fp32 vertices, fp32-rounded edge points and interior points of a random triangle of a random instance, from an origin
    10^[-1, 2] triangle sizes or instance sizes away --, half random through the instance's box. Directions normalised, scaled by 1e-3 / 1e3,
    or left as the difference; every 16th has a zero, a -0.0 or a 1e-30 component; a tenth carry a finite interval around the target."""
    world = world_triangles(soup)
    boxes = [(w.reshape(-1, 3).min(0), w.reshape(-1, 3).max(0)) for w in world]
    o = np.zeros((count, 3)); target = np.zeros((count, 3))
    for k in range(count):
        w = world[k % len(world)]
        t = w[rng.integers(len(w))]
        size = np.abs(t - t.mean(0)).max() + 1e-30
        lo, hi = boxes[k % len(world)]
        kind = k % 6
        if kind == 0:
            p = t[rng.integers(3)]
        elif kind == 1:
            s = rng.uniform(0.02, 0.98); e = rng.integers(3)
            p = t[e] + s * (t[(e + 1) % 3] - t[e])
        elif kind == 2:
            p = (rng.dirichlet((1, 1, 1))[:, None] * t).sum(0)
        else:
            p = rng.uniform(lo, hi)
        p = p.astype(f32).astype(f64)
        reach = size if kind < 3 and k % 4 else np.abs(hi - lo).max()
        o[k] = p + rng.normal(size=3) * reach * 10 ** rng.uniform(-1, 2)
        target[k] = p
    o = o.astype(f32)
    d = target - o.astype(f64)
    mode = np.arange(count) % 5
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where((mode < 2)[:, None], d / ln, np.where((mode == 2)[:, None], d * 1e-3, np.where((mode == 3)[:, None], d * 1e3, d))).astype(f32)
    special = np.nonzero(np.arange(count) % 16 == 7)[0]
    axis = rng.integers(0, 3, count)
    d[special, axis[special]] = np.array([0.0, -0.0, 1e-30, -1e-30], f32)[np.arange(len(special)) % 4]
    rays = I.rays_of(o, d)
    cut = np.arange(count) % 10 == 3                               # t of the target in the ray's own units: |target - o| / |d|
    tt = (ln[:, 0] / np.linalg.norm(d.astype(f64), axis=1))
    rays[cut, 3] = (tt[cut] * 0.5).astype(f32); rays[cut, 7] = (tt[cut] * 1.5).astype(f32)
    return rays


# ----------------------------------------------------------------------------------------------
# CPU: the oracle's own boxes, and the exact closest hit on a sample
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_oracle_bvh_equals_brute_force(oracle, name):
    soup, rays = hostile(name)
    assert max(sum(len(g) for g in geoms) for geoms in soup.nodes) <= 1500
    brute = I.oracle_closest(oracle, soup.scene, rays, accel_mode=0)
    tree = I.oracle_closest(oracle, soup.scene, rays, accel_mode=1)
    assert not I.same_records(tree, brute), name
    hits = float((brute["Instance"] != I.MISS).mean())
    assert hits > 0.15, f"{name}: only {hits:.1%} of the rays hit anything"
    sel = np.arange(0, len(rays), 389 if name == "instanced" else 97)          # six instances: every ray against 4 200 triangles
    fig = R.check_closest(rays[sel], soup.instances, brute[sel], soup.slot_of, f"oracle, {name}")
    print(f"[oracle] {name}: {hits:.1%} of {len(rays)} rays hit; exact closest on {len(sel)}: {fig}")


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
def box_plane_rays(lay, buf):
    """rays for the flat grid (plane y = 0) from origins exactly on child-box planes of its bottom level: in the plane along +-x and +-z
    and diagonally, and from above the plane straight down and slanted along an axis"""
    inst, nodes, tris, order = bvh_check.split(lay, buf)
    nb = int(inst[0]["nodeBase"])
    o, d = [], []
    for n in nodes[nb:nb + 48]:
        lo, hi = bvh_check.child_boxes(n)
        for s in range(8):
            if int(n["meta"][s]) == 0:
                continue
            for x, z in ((lo[s, 0], lo[s, 2]), (hi[s, 0], hi[s, 2]), (lo[s, 0], hi[s, 2])):
                for dd in ((1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (1, 0, 1), (-1, 0, 0.5)):
                    o.append((x, 0.0, z)); d.append(dd)
                for dd in ((0, -1, 0), (1, -1, 0), (0, -1, -1), (0, -0.0, 1)):
                    o.append((x, 0.75, z)); d.append(dd)
                o.append((x, hi[s, 1], z)); d.append((0.25, -1, 0.5))
    return I.rays_of(np.array(o, f32), np.array(d, f32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_walk_equals_brute_force(gpu, ptamd, oracle, pkg, name):
    soup, rays = hostile(name)
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, soup.scene)
    try:
        lay, buf = gpu.download_blob()
        bvh_check.check_blob(lay, buf, lambda n: 2 if n <= 32 else 1)
        if name == "flat_grid":
            rays = np.concatenate([rays, box_plane_rays(lay, buf)])
        gpu.reset_counters()
        walk = gpu.trace_closest(rays)
        brute = gpu.trace_closest(rays, brute_force=True)
        assert gpu.counters().StackOverflows == 0
        bad = I.same_records(walk, brute, I.FIELDS + ("Slot",))
        assert not bad, f"{name}: the walk and brute force differ: {bad}"
        bad = I.same_records(brute, I.oracle_closest(oracle, soup.scene, rays))
        assert not bad, f"{name}: the device and the oracle differ: {bad}"
        # one frame per schedule against the oracle's brute-force frame
        gs = S.graphics_settings(W, H, spp=1, bounces=3)
        ref_gb, ref_rays, ref_f32 = oracle.render(soup.scene, gs, accel_mode=0, want_f32=True, layouts=L)
        assert (ref_f32[..., :3] != ref_f32[0, 0, :3]).any(), "the camera sees nothing"
        r = ptamd.Renderer(gpu, g, W, H, with_f32=True)
        for flags in (0, 8, 4, 0x10):
            for t in r.textures.values():
                t.zero_()
            gpu.set_debug_flags(flags); gpu.reset_counters()
            try:
                r.render(gs); gpu.sync()
            finally:
                gpu.set_debug_flags(0)
            c = gpu.counters()
            out = ptamd.textures_to_numpy(r.textures)
            assert c.StackOverflows == 0 and c.PrimaryRays + c.SecondaryRays == ref_rays, (name, flags)
            assert np.array_equal(out["Position"].view(np.uint32), ref_gb["Position"].view(np.uint32)), (name, flags)
            assert np.array_equal(out["RadianceF32"].view(np.uint32), ref_f32.view(np.uint32)), (name, flags)
        gpu.set_debug_flags(2); gpu.reset_counters()
        try:
            r.render(gs); gpu.sync()
        finally:
            gpu.set_debug_flags(0)
        c = gpu.counters()
        assert c.SecondaryRays > 0 and c.BvhMismatches == 0 and c.StackOverflows == 0, name
    finally:
        g.close()
    print(f"[device] {name}: {float((walk['Instance'] != I.MISS).mean()):.1%} of {len(rays)} rays hit, walk = brute force = oracle")


# ----------------------------------------------------------------------------------------------
# a transform without an inverse
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def squashed():
    """an 80-triangle sphere, and the same sphere squashed flat by a zero scale along y: worldToObject of the second is inf / NaN"""
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L
    import dxpbrt_amd.scenes as S

    class P:
        layouts, scenes = L, S
    sphere = I.icosphere(P, 1)
    soup = I.Soup(P, ge.load_oracle(), [[sphere]], [(0, I.affine((1, 1, 1), (-1.5, 0, 3))), (0, I.affine((1, 0, 1), (1.5, 0.25, 3), 0.4))])
    rng = np.random.default_rng(15)
    o = rng.normal(size=(2000, 3)) * 4.0
    target = np.array([(-1.5, 0, 3), (1.5, 0.25, 3)])[np.arange(2000) % 2] + rng.uniform(-1, 1, (2000, 3))
    return soup, I.rays_of(o.astype(f32), (target - o).astype(f32))


def test_oracle_with_a_singular_instance(oracle):
    soup, rays = squashed()
    brute = I.oracle_closest(oracle, soup.scene, rays, accel_mode=0)
    assert not I.same_records(I.oracle_closest(oracle, soup.scene, rays, accel_mode=1), brute)
    hit = brute["Instance"] != I.MISS
    assert hit.mean() > 0.2 and (brute["Instance"][hit] == 0).all()          # no ray comes back through a transform without an inverse


@pytest.mark.gpu
def test_singular_instance_keeps_a_finite_box(gpu, ptamd, oracle):
    """instance_world_box pads by the magnitude of worldToObject's translation: where that is inf / NaN the flat world box must stay the
    finite box it was, the structure sound, and the walk what brute force and the oracle say"""
    soup, rays = squashed()
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, soup.scene)
    try:
        lay, buf = gpu.download_blob()
        inst = bvh_check.split(lay, buf)[0]
        assert not np.isfinite(inst["worldToObject"][1]).all()
        assert np.isfinite(inst["boxLo"]).all() and np.isfinite(inst["boxHi"]).all()
        assert (inst["boxHi"][1] - inst["boxLo"][1])[1] < 1e-3               # still flat
        bvh_check.check_blob(lay, buf, lambda n: 2 if n <= 32 else 1)
    finally:
        g.close()
    I.device_records(gpu, ptamd, soup, rays, "singular instance", I.oracle_closest(oracle, soup.scene, rays))
