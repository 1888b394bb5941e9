"""Input sets of tests/test_intersection_reference.py and tests/test_traversal_hostile.py: triangle soups as scenes.Scene objects, the same
soups as tests/isectref.py instance lists, and the rays that break intersection code. Everything is seeded; nothing here knows the fp32
recipe under test."""
import ctypes as C

import numpy as np

f32, f64 = np.float32, np.float64
MISS = 0xFFFFFFFF
FIELDS = ("T", "U", "V", "Instance", "Geometry", "Primitive")          # what the oracle and the device must agree on (Slot: packet order)


def identity():
    return np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)


def affine(scale=(1, 1, 1), translation=(0, 0, 0), yaw=0.0, pitch=0.0):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m = np.zeros((3, 4)); m[:, :3] = ry @ rx @ np.diag(scale); m[:, 3] = translation
    return m.astype(f32)


class Soup:
    """nodes: one bottom level each, a list of geometries [n, 3, 3] fp32; objects: (node, 3x4 objectToWorld). `scene` is what the device and
    the oracle take, `instances` what isectref takes (worldToObject by the oracle's or_invert_3x4: the project's definition of it)."""

    def __init__(self, pkg, oracle, nodes, objects, camera=None):
        S = pkg.scenes
        self.nodes = [[np.ascontiguousarray(g, f32).reshape(-1, 3, 3) for g in geoms] for geoms in nodes]
        self.objects = [(int(n), np.asarray(m, f32).reshape(3, 4)) for n, m in objects]
        mat = S.material()
        mesh_nodes = [S.MeshNode([S.Mesh(S.make_vertices(g.reshape(-1, 3)), S.make_indices(np.arange(g.size // 3)), False, mat) for g in geoms])
                      for geoms in self.nodes]
        cam = camera if camera is not None else S.make_camera((0, 0, -5), aspect=4 / 3)
        self.scene = S.Scene(mesh_nodes, [S.RenderObject(n, m) for n, m in self.objects], cam, S.make_scene_data((0.2, 0.3, 0.4, 1.0))).finalize()
        self.instances, self.offsets = [], []
        fp = C.POINTER(C.c_float)
        for n, m in self.objects:
            w2o = np.zeros(12, f32); mm = np.ascontiguousarray(m.reshape(12))
            oracle.lib().or_invert_3x4(mm.ctypes.data_as(fp), w2o.ctypes.data_as(fp))
            geoms = self.nodes[n]
            self.instances.append((w2o, np.concatenate(geoms), np.concatenate([np.full(len(g), k, np.uint32) for k, g in enumerate(geoms)]),
                                   np.concatenate([np.arange(len(g), dtype=np.uint32) for g in geoms])))
            self.offsets.append(np.cumsum([0] + [len(g) for g in geoms]))

    def slot_of(self, x, geom, prim):
        return self.offsets[x][np.asarray(geom, np.int64)] + np.asarray(prim, np.int64)

    def only(self, x):
        """the instance list with every instance but x emptied (isectref skips those)"""
        return [inst if k == x else (inst[0], inst[1][:0], inst[2][:0], inst[3][:0]) for k, inst in enumerate(self.instances)]


def rays_of(o, d, tmin=0.0, tmax=np.inf):
    o = np.asarray(o, f32); r = np.zeros((len(o), 8), f32)
    r[:, 0:3] = o; r[:, 3] = tmin; r[:, 4:7] = np.asarray(d, f32); r[:, 7] = tmax
    return r


def oracle_closest(oracle, scene, rays, accel_mode=0):
    osc = oracle.OracleScene(scene, accel_mode=accel_mode)
    rays = np.ascontiguousarray(rays, f32)
    rec = np.zeros(len(rays) * 32, np.uint8)
    oracle.lib().or_trace_closest(osc.handle, rays.ctypes.data, len(rays), rec.ctypes.data)
    osc.close()
    from isectref import RECORD
    return rec.view(RECORD)


def oracle_visibility(oracle, scene, rays):
    osc = oracle.OracleScene(scene, accel_mode=0)
    rays = np.ascontiguousarray(rays, f32)
    out = np.zeros((len(rays), 4), f32)
    oracle.lib().or_trace_visibility(osc.handle, rays.ctypes.data, len(rays), out.ctypes.data)
    osc.close()
    return out


def oracle_pairs(oracle, o, d, v0, v1, v2, tmin=-np.inf, tmax=np.inf):
    """or_ray_triangle per pair: hit, t, u, v"""
    lib = oracle.lib()
    arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, f32), np.asarray(v0).shape)) for x in (o, d, v0, v1, v2)]
    n = len(arrs[0])
    hit = np.zeros(n, bool); out = np.zeros((3, n), f32)
    fp = C.POINTER(C.c_float)
    t, u, v = C.c_float(), C.c_float(), C.c_float()
    base = [a.ctypes.data for a in arrs]
    for i in range(n):
        p = [C.cast(b + 12 * i, fp) for b in base]
        if lib.or_ray_triangle(p[0], p[1], tmin, tmax, p[2], p[3], p[4], C.byref(t), C.byref(u), C.byref(v)):
            hit[i] = True; out[0, i], out[1, i], out[2, i] = t.value, u.value, v.value
    return hit, out[0], out[1], out[2]


def same_records(a, b, fields=FIELDS):
    """fields of two record arrays that differ in a bit (T, U, V as bit patterns), with the first differing row"""
    bad = []
    for n in fields:
        x, y = np.ascontiguousarray(a[n]).view(np.uint32), np.ascontiguousarray(b[n]).view(np.uint32)
        if not np.array_equal(x, y):
            i = int(np.nonzero(x != y)[0][0])
            bad.append((n, int((x != y).sum()), i, a[n][i], b[n][i]))
    return bad


def device_records(gpu, ptamd, soup, rays, what, oracle_rec=None):
    """pt_debug_trace_closest through the walk and through brute force over a freshly built scene: the two must agree in every field, the
    brute-force one with the oracle's in FIELDS, and no push may have been refused"""
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, soup.scene)
    try:
        gpu.reset_counters()
        walk = gpu.trace_closest(rays)
        brute = gpu.trace_closest(rays, brute_force=True)
        assert gpu.counters().StackOverflows == 0, what
    finally:
        g.close()
    bad = same_records(walk, brute, FIELDS + ("Slot",))
    assert not bad, f"{what}: the walk and brute force differ: {bad}"
    if oracle_rec is not None:
        bad = same_records(brute, oracle_rec)
        assert not bad, f"{what}: the device and the oracle differ: {bad}"
    return walk


# ----------------------------------------------------------------------------------------------
# random pairs, dominant axes, exact zeros
# ----------------------------------------------------------------------------------------------
def random_pairs(n=12000, seed=1):
    """triangles of scale 10^[-2, 2] around offsets up to 1e3, rays from a few scales away aimed at barycentric targets in [-0.2, 1.4];
    the first half of the directions normalised, the rest left at the distance to the target (t ~ 1)"""
    rng = np.random.default_rng(seed)
    scale = 10 ** rng.uniform(-2, 2, n)
    off = rng.uniform(-1, 1, (n, 3)) * 10 ** rng.uniform(0, 3, (n, 1))
    v = (rng.normal(size=(n, 3, 3)) * scale[:, None, None] + off[:, None, :]).astype(f32)
    b = rng.uniform(-0.2, 1.4, (n, 2))
    target = v[:, 0].astype(f64) * (1 - b[:, :1] - b[:, 1:]) + v[:, 1] * b[:, :1] + v[:, 2] * b[:, 1:]
    o = (target + rng.normal(size=(n, 3)) * scale[:, None] * 10 ** rng.uniform(-0.5, 1, (n, 1))).astype(f32)
    d = target - o
    d[:n // 2] /= np.linalg.norm(d[:n // 2], axis=1, keepdims=True)
    return o, d.astype(f32), v


def dominant_axis_pairs(seed=2, per_case=60):
    """Every dominant axis with either sign, and the ties |dx| == |dy|, |dy| == |dz|, |dx| == |dz| and all three, with all sign patterns.
    Geometry on a quarter-integer lattice so that rays through vertices and edge points are exact: those take the fallback."""
    rng = np.random.default_rng(seed)
    cases = []
    for axis in range(3):
        for sign in (1, -1):
            for _ in range(per_case):
                d = rng.integers(-7, 8, 3).astype(f64)
                d[axis] = sign * (np.abs(d).max() + rng.integers(1, 4))
                cases.append(d)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        for sa in (1, -1):
            for sb in (1, -1):
                for _ in range(per_case // 2):
                    m = rng.integers(2, 9)
                    d = rng.integers(-m, m + 1, 3).astype(f64)
                    d[a], d[b] = sa * m, sb * m
                    cases.append(d)
    for s in np.array(np.meshgrid((1, -1), (1, -1), (1, -1))).reshape(3, -1).T:
        for m in (1, 3, 5):
            cases.append(s.astype(f64) * m)
    d = np.array(cases)
    n = len(d)
    o = rng.integers(-8, 9, (n, 3)).astype(f64) / 4
    hitp = o + d                                                    # the aimed point: t = 1
    e1, e2 = rng.integers(-12, 13, (n, 3)) / 4.0, rng.integers(-12, 13, (n, 3)) / 4.0
    kind = np.arange(n) % 4                                         # 0 interior, 1 through v0, 2 on the edge v0-v1, 3 a near miss beyond that edge
    bu = np.where(kind == 0, 0.25, np.where(kind == 2, 0.5, 0.0))
    bv = np.where(kind == 0, 0.25, np.where(kind == 3, -0.125, 0.0))
    v0 = hitp - bu[:, None] * e1 - bv[:, None] * e2                 # hitp = v0 + bu e1 + bv e2, exact on the lattice
    v = np.stack([v0, v0 + e1, v0 + e2], 1)
    scale = np.where(np.arange(n) % 3 == 0, 1.0, np.where(np.arange(n) % 3 == 1, 0.125, 8.0))    # the normalised half is not exact; these stay so
    half = np.arange(n) % 2 == 1
    df = (d * scale[:, None]).astype(f32)
    df[half] = (d[half] / np.linalg.norm(d[half], axis=1, keepdims=True)).astype(f32)
    # a normalised direction keeps its ties only where the two components round alike: they do (same magnitude, same rounding)
    return o.astype(f32), df, v.astype(f32)


def grid_mesh(n=6, z=4.0):
    """n x n quads on the integer lattice at height z, two triangles per quad: (tris [2 n n, 3, 3], incident(x, y) -> triangles at a point)"""
    tris = []
    for j in range(n):
        for i in range(n):
            p = [(i, j, z), (i + 1, j, z), (i + 1, j + 1, z), (i, j + 1, z)]
            tris += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    return np.array(tris, f32)


def incident(tris, p):
    """indices of the triangles of a z-plane mesh whose closed 2D extent contains p exactly (float64 on quarter-integers: exact)"""
    a, b, c = (tris[:, k, :2].astype(f64) for k in range(3))
    p = np.asarray(p, f64)[:2]
    cr = lambda u, w: u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    e = np.stack([cr(b - a, p - a), cr(c - b, p - b), cr(a - c, p - c)], 1)
    return np.nonzero((e >= 0).all(1) | (e <= 0).all(1))[0]


def exact_zero_rays(tris, n=6, z=4.0):
    """rays from integer origins on both sides of the plane to every interior lattice vertex (all edge functions of the incident triangles
    are exactly 0 where they should be), then to points at quarters of interior edges: (o, d, list of incident triangle indices)"""
    o, d, inc = [], [], []
    origins = [(x, y, zz) for zz in (z - 4, z - 3, z - 1, z + 1, z + 2, z + 8) for x in (-2, 1, 3, 7) for y in (-1, 2, 4, 9)]
    targets = [(i, j) for i in range(1, n) for j in range(1, n)]
    for tx, ty in targets:
        who = incident(tris, (tx, ty))
        for og in origins:
            o.append(og); d.append((tx - og[0], ty - og[1], z - og[2])); inc.append(who)
    edge_points = [(i + q, j) for i in range(1, n - 1) for j in range(1, n) for q in (0.25, 0.5)] + \
                  [(i, j + q) for i in range(1, n) for j in range(1, n - 1) for q in (0.25, 0.75)] + \
                  [(i + q, j + q) for i in range(1, n - 1) for j in range(1, n - 1) for q in (0.25, 0.5)]
    for k, (tx, ty) in enumerate(edge_points):
        who = incident(tris, (tx, ty))
        for og in origins[k % 7::7]:
            o.append(og); d.append((tx - og[0], ty - og[1], z - og[2])); inc.append(who)
    return np.array(o, f32), np.array(d, f32), inc


def in_plane_rays(n=6, z=4.0):
    """rays that travel exactly in the mesh's plane, along lattice lines, diagonals and in between: every edge value and det are exactly 0"""
    o, d = [], []
    for k in range(0, n + 1):
        o += [(-2, k, z), (k, -3, z), (-1, k - 1, z), (8, k, z), (k + 0.5, -2, z)]
        d += [(1, 0, 0), (0, 1, 0), (1, 1, 0), (-3, 1, 0), (0.25, 2, 0)]
    return np.array(o, f32), np.array(d, f32)


# ----------------------------------------------------------------------------------------------
# closed meshes
# ----------------------------------------------------------------------------------------------
def icosphere(pkg, subdiv):
    m = pkg.scenes.icosphere_mesh(subdiv, None)
    return m.vertices["Position"][m.indices.astype(np.int64)].reshape(-1, 3, 3).astype(f32)


def tetrahedron():
    p = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], f32) * f32(0.75)
    return p[np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])]


# name -> (unit triangles, closed); the open ones are the first n triangles of the 80-triangle sphere (the sizes at which
# blas_leaf_tris and the single-leaf root change: 2 | 3 and 32 | 33)
def unit_meshes(pkg):
    out = {f"ico{20 * 4 ** s}": (icosphere(pkg, s), True) for s in range(4)}
    out["tetra"] = (tetrahedron(), True)
    for n in (1, 2, 3, 32, 33):
        out[f"patch{n}"] = (icosphere(pkg, 1)[:n].copy(), False)
    return out


def placed(unit, scale, centre):
    """vertices scaled and moved in float64, rounded once: the mesh stays closed because shared vertices round alike"""
    return (unit.astype(f64) * scale + np.asarray(centre, f64)).astype(f32)


def aimed_rays(tris, closed, centre, radius, count, rng):
    """Rays from random points near `centre` (inside the mesh) at fp32 vertices and at fp32-rounded points on edges of `tris` (world
    space). An open patch takes only vertices and edges that are interior to it (shared by two of its triangles / surrounded), plus
    points well inside its triangles. Half normalised, the others scaled by 1e-3 or 1e3; every eighth ray has one component of its
    direction exactly zero, written as -0.0 or 1e-30."""
    t64 = tris.astype(f64)
    edges = {}
    for ti, t in enumerate(tris):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            key = tuple(sorted((t[a].tobytes(), t[b].tobytes())))
            edges.setdefault(key, []).append((ti, a, b))
    shared = [v[0] for v in edges.values() if len(v) == 2]
    targets = []
    if closed:
        verts = np.unique(tris.reshape(-1, 3), axis=0).astype(f64)
    else:
        # a vertex is interior when every edge at it is shared
        open_pts = {k for key, v in edges.items() if len(v) == 1 for k in key}
        verts = np.array([p for p in np.unique(tris.reshape(-1, 3), axis=0) if p.tobytes() not in open_pts], f64).reshape(-1, 3)
    for k in range(count):
        kind = k % 3
        if kind == 0 and len(verts):
            p = verts[rng.integers(len(verts))]
        elif kind == 1 and len(shared):
            ti, a, b = shared[rng.integers(len(shared))]
            s = rng.uniform(0.02, 0.98)
            p = (t64[ti, a] + s * (t64[ti, b] - t64[ti, a])).astype(f32).astype(f64)
        else:
            ti = rng.integers(len(tris)); w = rng.dirichlet((1, 1, 1)) * 0.7 + 0.1
            p = (w[:, None] * t64[ti]).sum(0).astype(f32).astype(f64)
        targets.append(p)
    targets = np.array(targets)
    o = np.asarray(centre, f64) + rng.uniform(-1, 1, (count, 3)) * radius
    # every eighth ray travels in an axis plane: one component of its direction is exactly 0. Inside a closed mesh any such direction
    # must hit; at an open patch the ray is aimed at a point well inside a triangle from an origin moved into that point's plane
    zero = np.arange(count) % 8 == 5
    axis = rng.integers(0, 3, count)
    for k in np.nonzero(zero)[0]:
        if closed:
            targets[k] = o[k] + rng.normal(size=3) * radius
        else:
            ti = rng.integers(len(tris)); w = rng.dirichlet((1, 1, 1)) * 0.7 + 0.1
            targets[k] = (w[:, None] * t64[ti]).sum(0).astype(f32).astype(f64)
    o = o.astype(f32)
    if closed:
        targets[zero, axis[zero]] = o[zero, axis[zero]]
    else:
        o[zero, axis[zero]] = targets[zero, axis[zero]].astype(f32)
    d = targets - o.astype(f64)
    mode = np.arange(count) % 4                                     # 0, 2: normalised; 1: x 1e-3; 3: x 1e3
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where((mode % 2 == 0)[:, None], d / ln, d * np.where(mode == 1, 1e-3, 1e3)[:, None]).astype(f32)
    tiny = np.where(np.arange(count) % 16 == 5, f32(-0.0), f32(1e-30))
    d[zero, axis[zero]] = tiny[zero]
    return o, d


PLACEMENTS = {"unit": (1.0, (0.0, 0.0, 0.0)), "far_small": (0.01, (1000.25, -333.5, 77.125)), "huge": (1e3, (3.0, 4.0, 5.0))}
INSTANCED = [affine((-1, 1, 1), (2, 1, -3), 0.7, 0.3), affine((1e-3, 1e-3, 1e-3), (0.5, -0.25, 2.0), 1.1, -0.4),
             affine((1e3, 1e3, 1e3), (-700.0, 250.0, 3000.0), -0.6, 0.2), affine((1, -1.5, 0.5), (-4, 0, 1), 2.0, 1.0)]


def closed_mesh_sets(pkg, oracle, rays_per_mesh=300, seed=4):
    """[(name, Soup, rays [m, 8], expected instance per ray)]: one scene per placement with every mesh of unit_meshes as an instance of its
    own, side by side; `instanced` puts the unit meshes through mirrored, 1e-3, 1e3 and sheared-scale instance transforms instead."""
    meshes = unit_meshes(pkg)
    rng = np.random.default_rng(seed)
    out = []
    for pname, (scale, centre) in PLACEMENTS.items():
        nodes, objects, rays, expect = [], [], [], []
        for k, (mname, (unit, closed)) in enumerate(meshes.items()):
            c = np.asarray(centre, f64) + np.array([4.0 * scale * k, 0, 0])
            tris = placed(unit, scale, c)
            nodes.append([tris]); objects.append((k, identity()))
            o, d = aimed_rays(tris, closed, c, 0.2 * scale, rays_per_mesh, rng)      # inside the tetrahedron too (inradius 0.43)
            rays.append(rays_of(o, d)); expect.append(np.full(len(o), k))
        out.append((pname, Soup(pkg, oracle, nodes, objects), np.concatenate(rays), np.concatenate(expect)))
    nodes, objects, rays, expect = [], [], [], []
    for k, (mname, (unit, closed)) in enumerate(meshes.items()):
        m = INSTANCED[k % len(INSTANCED)].copy()
        m[:, 3] += (m[:, :3].astype(f64) @ np.array([4.0 * k, 0, 0])).astype(f32)
        nodes.append([unit]); objects.append((k, m))
        world = (unit.astype(f64) @ m[:, :3].astype(f64).T + m[:, 3].astype(f64)).astype(f32)
        c = m[:, 3].astype(f64)
        radius = 0.1 * np.abs(np.linalg.det(m[:, :3].astype(f64))) ** (1 / 3)
        o, d = aimed_rays(world, closed, c, radius, rays_per_mesh, rng)
        rays.append(rays_of(o, d)); expect.append(np.full(len(o), k))
    out.append(("instanced", Soup(pkg, oracle, nodes, objects), np.concatenate(rays), np.concatenate(expect)))
    return out


# ----------------------------------------------------------------------------------------------
# closest of many, duplicates
# ----------------------------------------------------------------------------------------------
def duplicate_soup(pkg, oracle, seed=5, n=48):
    """One bottom level of two geometries: geometry 0 holds n random triangles of which the last n / 4 repeat the first n / 4, geometry 1
    repeats every third triangle of geometry 0. Instances 0 and 1 carry it under the same transform, instance 2 under another."""
    rng = np.random.default_rng(seed)
    base = (rng.normal(size=(n - n // 4, 1, 3)) * 1.5 + rng.normal(size=(n - n // 4, 3, 3)) * 0.8).astype(f32)
    g0 = np.concatenate([base, base[:n // 4]])
    g1 = g0[::3].copy()
    m = affine((1.5, 1.0, 0.75), (0.25, -0.5, 1.0), 0.4, -0.2)
    soup = Soup(pkg, oracle, [[g0, g1]], [(0, m), (0, m), (0, affine((1, 1, 1), (0.5, 0.5, 0.5), -1.0, 0.3))])
    world = (np.concatenate([g0, g1]).astype(f64) @ m[:, :3].astype(f64).T + m[:, 3])
    k = 600
    ti = rng.integers(len(world), size=k)
    w = rng.dirichlet((1, 1, 1), k)
    target = (w[:, :, None] * world[ti]).sum(1)
    o = target + rng.normal(size=(k, 3)) * 6.0
    d = target - o
    d[::2] /= np.linalg.norm(d[::2], axis=1, keepdims=True)
    return soup, rays_of(o.astype(f32), d.astype(f32))


def lowest_identical(soup, rec):
    """for every hit record the lowest (instance, geometry, primitive) among the triangles that are bit-identical to the reported one under
    a bit-identical transform -- the id the closest-hit rule must report -- and how many such copies there are"""
    want = np.stack([rec["Instance"], rec["Geometry"], rec["Primitive"]], 1).astype(np.int64)
    copies = np.zeros(len(rec), np.int64)
    for r in np.nonzero(rec["Instance"] != MISS)[0]:
        x = int(rec["Instance"][r])
        tri = soup.instances[x][1][int(soup.slot_of(x, rec["Geometry"][r], rec["Primitive"][r]))].tobytes()
        ids = []
        for y, (w2o, tris, geom, prim) in enumerate(soup.instances):
            if soup.objects[y][1].tobytes() == soup.objects[x][1].tobytes():
                ids += [(y, int(geom[j]), int(prim[j])) for j in range(len(tris)) if tris[j].tobytes() == tri]
        want[r] = min(ids); copies[r] = len(ids)
    return want, copies


def ulp_steps(t):
    t = np.asarray(t, f32)
    return np.nextafter(t, f32(-np.inf)), np.nextafter(t, f32(np.inf))
