"""Deep trees for tests/test_deep_trees_rules.py and tests/test_deep_trees_gpu.py: meshes and instance fields on which the builder's
Morton keys give a wide tree of 17 to 24 levels, the depths bvhref.build predicts for them, rays that run down those trees, and a
host model of the one-lane walk (trace_single, csrc/pt_trace2.hpp) that writes and replays the step log of pt_debug_trace_ray.

nested_shells: start from the unit cube; shell k halves the current cell along axis k % 3, scatters m small triangles through the upper
half and continues in the lower half. Every shell differs from the rest in one more leading bit of a Morton key, so the radix tree is a
comb and the collapse cannot flatten it: the depth grows with the number of shells, not with the number of triangles. The same
construction over small tetrahedra as instances gives a deep top level. (A geometric progression of single triangles stops at depth 9.)

Scenes (SPECS): what each is for, with the depths predicted on the CPU; tests/test_deep_trees_rules.py asserts them without a GPU.

The log: trace_single appends (code, a, b, sp) per step --
  1  enter instance a; b = T.y still to enter; then G, T and a marker are pushed (sp is logged before the three pushes)
  2  test triangle b of instance a
  3  visit: (a, b) = G before the visit; the highest hit bit is taken off and the rest of G is pushed when it still names a hit child
  4  the fetched node's groups: a = G.y (hit internal children << 24 | imask), b = T.y
  5  pop: (a, b) = the entry, sp after the pop
  6  a marker was popped: T and G of the top level are popped after it; (a, b) = (G.y, T.y) restored
  7  end: (instance, packet) of the closest hit
replay() runs a model stack along such a log and demands that every pop returns what the matching push left, that sp is the model's
depth at every step, that the parked top-level state comes back, and that the walk ends with an empty stack."""
import functools

import numpy as np

import bvh_check
import isectsets as I

f32, f64 = np.float32, np.float64
MARKER = (0xFFFFFFFF, 0)
LDS_DEPTH = 12                       # kLdsStackDepth (pt_shade.hpp) = kStreamStackLds (pt_stream.hip)
STACK_SIZE = 64                      # kStackSize (pt_trace.hpp)
STACK_LDS_FLAT, STACK_LDS_PHASED = 4, 8          # kStackLdsFlat (pt_trace2.hpp), kStackLds2 (pt_kernels.hip)
BLOB_LDS_MAX = 40 * 1024             # kBlobLdsMax (pt_kernels.hip): a traversal copy up to here is staged in LDS
SINGLE_GROUP_LEAVES = 4096           # kSingleGroupCollapseLeaves (pt_bvh.hip)
W, H = 64, 48


# ----------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------
def shell_cells(nshell):
    """([(lo, hi)] of the upper half of every shell, (lo, hi) of the cell that is left over)"""
    lo, hi = np.zeros(3), np.ones(3)
    out = []
    for k in range(nshell):
        a = k % 3
        mid = 0.5 * (lo[a] + hi[a])
        ulo = lo.copy(); ulo[a] = mid
        out.append((ulo, hi.copy()))
        hi = hi.copy(); hi[a] = mid
    return out, (lo.copy(), hi.copy())


def shell_points(nshell, m, seed):
    """m centres per shell over 90 % of its half-cell: (centres [nshell, m, 3], extents [nshell, 3], cells)"""
    rng = np.random.default_rng(seed)
    cells, rest = shell_cells(nshell)
    centres = np.array([0.5 * (lo + hi) + rng.uniform(-0.45, 0.45, (m, 3)) * (hi - lo) for lo, hi in cells])
    return centres, np.array([hi - lo for lo, hi in cells]), cells, rest, rng


def nested_shells(nshell, m, seed=0):
    """-> (triangles [nshell * m, 3, 3] float32, shell of every triangle). Vertices jitter by 2 % of the half-cell's extent around the
    centre and are clipped into the half-cell."""
    centres, ext, cells, rest, rng = shell_points(nshell, m, seed)
    tris = np.zeros((nshell, m, 3, 3))
    for k, (lo, hi) in enumerate(cells):
        v = centres[k][:, None, :] + rng.uniform(-1, 1, (m, 3, 3)) * 0.02 * ext[k]
        tris[k] = np.clip(v, lo, hi)
    return tris.reshape(-1, 3, 3).astype(f32), np.repeat(np.arange(nshell), m)


def jittered_shells(nshell, m, seed=0, jitter_seed=1):
    """nested_shells with every vertex moved by up to half a percent of its half-cell's extent, still inside the half-cell"""
    tris, shell = nested_shells(nshell, m, seed)
    rng = np.random.default_rng(jitter_seed)
    cells, _ = shell_cells(nshell)
    lo, hi = np.array([c[0] for c in cells])[shell], np.array([c[1] for c in cells])[shell]
    moved = tris.astype(f64) + rng.uniform(-1, 1, tris.shape) * 0.005 * (hi - lo)[:, None, :]
    return np.clip(moved, lo[:, None, :], hi[:, None, :]).astype(f32)


def nested_instances(nshell, m, seed=0):
    """3x4 transforms of nshell * m small tetrahedra placed like the triangles of nested_shells, and the cell left over"""
    centres, ext, cells, rest, rng = shell_points(nshell, m, seed)
    out = []
    for k in range(nshell):
        for c in centres[k]:
            s = 0.02 * ext[k]
            out.append(I.affine(s, np.clip(c, cells[k][0] + s, cells[k][1] - s)))
    return out, rest


def into_cell(cell, fill=0.9):
    """the transform that puts the unit cube into the middle `fill` of a cell"""
    lo, hi = cell
    return I.affine(fill * (hi - lo), lo + 0.5 * (1 - fill) * (hi - lo))


# name -> bottom-level shells x m, top-level shells x m (None: one instance under the identity). Depths as predicted_depths() gives them:
#   deep_small      top 0, bottom 19, 38 KB: the traversal copy is staged in LDS
#   deep_large      top 0, bottom 25, 4410 leaves: the per-level collapse, the streaming form
#   deep_two_level  top 13, bottom 17: 2 * (13 + 17) + 4 = 64, the deepest structure check_depth accepts. The fine-end rays enter the deep
#                   instance with (mostly) 9 or 10 entries on the stack: G, T and the marker end at entry 11, the last in LDS, or the marker is
#                   the first entry of the private part
#   too_deep        top 14, bottom 17: 66, the shallowest structure that is refused
#   deeper_mesh     the bottom level (19) that pt_update_bottom_level puts in the place of deep_two_level's: 2 * (13 + 19) + 4 = 68
SPECS = {
    "deep_small": dict(blas=(63, 7), tlas=None),
    "deep_large": dict(blas=(63, 70), tlas=None),
    "deep_two_level": dict(blas=(54, 16), tlas=(45, 6)),
    "too_deep": dict(blas=(54, 16), tlas=(48, 6)),
    "deeper_mesh": dict(blas=(60, 16), tlas=(45, 6)),
}


def geometry(name):
    """(meshes: [triangles] per bottom level, objects: [(mesh, 3x4)]) of a scene. Two-level scenes: the tetrahedra are mesh 0, the deep
    mesh is mesh 1 and its instance comes last, inside the innermost cell."""
    spec = SPECS[name]
    deep, _ = nested_shells(*spec["blas"])
    if spec["tlas"] is None:
        return [deep], [(0, I.identity())]
    xf, rest = nested_instances(*spec["tlas"])
    return [I.tetrahedron(), deep], [(0, m) for m in xf] + [(1, into_cell(rest))]


def wide_depth(nodes, single_leaf=False):
    """levels of a wide tree given as node records, the root first (the count accel_stats() and bvhref.check report: a root alone is 1,
    a tree of one leaf 0)"""
    if single_leaf:
        return 0
    depth, level = 0, [0]
    while level:
        depth += 1
        nxt = []
        for w in level:
            n = nodes[w]
            nxt += [int(n["childBase"]) + r for r in range(bin(int(n["imask"])).count("1"))]
        level = nxt
    return depth


def blas_depth(tris):
    """(depth, node count) of the bottom level bvhref.build makes of the triangles"""
    import bvhref
    from test_bvh_builder_rules import blas_params
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    nodes, _, T, _ = bvhref.build(tris.min(1), tris.max(1), blas_params(len(tris)))
    return wide_depth(nodes, T.nleaves <= 1), len(nodes)


@functools.lru_cache(None)
def assembled(name):
    """the scene as a hand-assembled traversal copy (test_bvh_builder_rules.assemble): (layout, buf, trees)"""
    from test_bvh_builder_rules import assemble
    meshes, objects = geometry(name)
    return assemble(meshes, objects)


@functools.lru_cache(None)
def predicted_depths(name):
    """(top-level depth, deepest bottom level) as bvhref.build with the restated blas_params / TLAS makes them: what accel_stats() must
    report, and what check_depth (pt_api.hip) adds up as 2 * (t + b) + 4. One instance is a top level of one leaf: depth 0."""
    meshes, objects = geometry(name)
    if len(objects) == 1:
        return 0, blas_depth(meshes[0])[0]
    lay, buf, trees = assembled(name)
    inst, nodes, tris, order = bvh_check.split(lay, buf)
    b = 0
    for it in inst:
        tc = int(it["triCount"])
        b = max(b, wide_depth(nodes[int(it["nodeBase"]):], tc <= (2 if tc <= 32 else 1)))
    return wide_depth(nodes), b


def stack_budget(name):
    t, b = predicted_depths(name)
    return 2 * (t + b) + 4


# ----------------------------------------------------------------------------------------------
# scenes and rays
# ----------------------------------------------------------------------------------------------
def world_triangles(meshes, objects):
    return [meshes[n].astype(f64) @ np.asarray(m, f64)[:, :3].T + np.asarray(m, f64)[:, 3] for n, m in objects]


RAYS = 4000
LOGGED = 64
# A ray from the origin corner passes through the upper half of EVERY shell only if dx <= dy <= dz <= 2 dx (shell 3j needs y, z <= 2 x
# where x is in the upper half, shell 3j + 1 needs x <= y and z <= 2 y, shell 3j + 2 needs x, y <= z); along (1, 1, 1) two shells of three
# are missed. The fine-end rays are drawn around that cone, leaning to z: on a map of the host walk's deepest sp over dy / dx and dz / dy
# (500 rays over the assembled deep_small) every ray with dz / dy >= 1.7 reached 16, a third of those with dz / dy around 1.3 did.


@functools.lru_cache(None)
def deep_rays(name, count=RAYS, seed=31):
    """[count, 8] rays (isectsets.rays_of layout) and their kind: 0 along the nesting diagonal from the coarse end, 1 from the fine end
    (both with small random tilts), 2 aimed at vertices, edge points and interiors of triangles of the innermost eight shells from
    10^[-1, 2] cell sizes away, 3 random through the scene box; and the distance to every ray's target in units of its direction. Every 16th ray has a zero, -0.0 or +-1e-30 direction component, a tenth
    carry a finite (tmin, tmax) around the target, as test_traversal_hostile.hostile_rays does."""
    spec = SPECS[name]
    meshes, objects = geometry(name)
    rng = np.random.default_rng(seed)
    ns, m = spec["blas"]
    world = world_triangles(meshes, objects)[-1]                    # the deep mesh in world space
    shell = np.repeat(np.arange(ns), m)
    inner = world[shell >= ns - 8]
    cell = np.abs(inner.reshape(-1, 3).max(0) - inner.reshape(-1, 3).min(0)).max()      # size of the innermost eight shells
    fine = inner.reshape(-1, 3).mean(0)
    M = np.asarray(objects[-1][1], f64)
    corner, scale = M[:, 3], np.diag(M[:, :3])                      # where the deep mesh's unit cube lies in the world
    finest = scale * 0.5 ** (ns // 3)
    kind = np.array([0, 2, 0, 3, 1, 2, 0, 3])[np.arange(count) % 8]
    o = np.zeros((count, 3)); target = np.zeros((count, 3))
    for k in range(count):
        if kind[k] == 0:
            o[k] = 1.0 + rng.uniform(0.05, 0.6, 3)
            target[k] = fine + rng.normal(size=3) * cell * 10 ** rng.uniform(-2, 0.5)
        elif kind[k] == 1:
            o[k] = corner - finest * rng.uniform(0.2, 3.0, 3)
            dy = 2.0 ** rng.uniform(0.3, 1.0); dz = dy * 2.0 ** rng.uniform(0.8, 1.2)
            target[k] = corner + scale * np.array([1.0, dy, dz]) / dz * rng.uniform(0.5, 1.0)
        elif kind[k] == 2:
            t = inner[rng.integers(len(inner))]
            which = rng.integers(3)
            if which == 0:
                p = t[rng.integers(3)]
            elif which == 1:
                s = rng.uniform(0.02, 0.98); e = rng.integers(3)
                p = t[e] + s * (t[(e + 1) % 3] - t[e])
            else:
                p = (rng.dirichlet((1, 1, 1))[:, None] * t).sum(0)
            target[k] = p.astype(f32).astype(f64)
            size = np.abs(t - t.mean(0)).max() * 25.0               # the triangle's half-cell: the jitter is 2 % of it
            o[k] = target[k] + rng.normal(size=3) * size * 10 ** rng.uniform(-1, 2)
        else:
            o[k] = rng.uniform(-0.3, 1.3, 3)
            target[k] = rng.uniform(0.0, 1.0, 3) * 0.5 ** rng.integers(0, 12)
    o = o.astype(f32)
    d = target - o.astype(f64)
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    mode = (np.arange(count) // 8) % 3
    d = np.where((mode == 0)[:, None], d / ln, np.where((mode == 1)[:, None], d, d * 1e3)).astype(f32)
    special = np.nonzero(np.arange(count) % 16 == 7)[0]
    axis = rng.integers(0, 3, count)
    d[special, axis[special]] = np.array([0.0, -0.0, 1e-30, -1e-30], f32)[np.arange(len(special)) % 4]
    rays = I.rays_of(o, d)
    cut = np.arange(count) % 10 == 3
    tt = ln[:, 0] / np.linalg.norm(d.astype(f64), axis=1)
    rays[cut, 3] = (tt[cut] * 0.5).astype(f32); rays[cut, 7] = (tt[cut] * 1.5).astype(f32)
    return rays, kind, tt.astype(f32)


def visibility_rays(name):
    """the same rays for the any-hit walk: every interval ends at one and a half times the distance to the ray's target"""
    rays, kind, tt = deep_rays(name)
    out = rays.copy()
    out[:, 7] = np.where(np.isfinite(rays[:, 7]), rays[:, 7], tt * f32(1.5))
    return out


def logged_rays(name):
    """indices of the LOGGED rays that go through pt_debug_trace_ray: rays from the fine end (the far children of every level are still
    owed while the walk goes down the near one: these are the rays whose stacks grow), then aimed ones; all with an open interval and no
    zero component (k_debug_trace rotates the direction by an angle of 0 for the logged lane, which may flip the sign of a zero)"""
    rays, kind, _ = deep_rays(name)
    plain = (rays[:, 3] == 0) & np.isinf(rays[:, 7]) & (np.abs(rays[:, 4:7]) > 1e-20).all(1)
    a = np.nonzero(plain & (kind == 1))[0][:LOGGED * 3 // 4]
    b = np.nonzero(plain & (kind == 2))[0][:LOGGED - len(a)]
    return np.concatenate([a, b])


@functools.lru_cache(None)
def scene(name):
    """(Soup, rays [RAYS, 8]) of a scene. The camera sits where the fine-end rays start and looks along them: every shell is in view at
    its own scale (a triangle is 2 % of its shell's distance: a few pixels), and the primary rays are rays whose stacks grow."""
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L
    import dxpbrt_amd.scenes as S

    class P:
        layouts, scenes = L, S
    meshes, objects = geometry(name)
    M = np.asarray(objects[-1][1], f64)
    finest = np.diag(M[:, :3]) * 0.5 ** (SPECS[name]["blas"][0] // 3)
    cam = S.make_camera(tuple((M[:, 3] - finest).tolist()), forward=(1.0, 1.6, 3.2), hfov_deg=40.0, aspect=W / H, near=1e-9)
    soup = I.Soup(P, ge.load_oracle(), [[mesh] for mesh in meshes], objects, cam)
    return soup, deep_rays(name)[0]


# ----------------------------------------------------------------------------------------------
# the one-lane walk on the host: the log it writes
# ----------------------------------------------------------------------------------------------
class ModelStack:
    """GroupStack<LDS_DEPTH> of pt_trace.hpp over plain memory: entries below lds_depth in one array, deeper ones in another, at
    sp - lds_depth. fault damages ONE thing (tests/test_deep_trees_rules.py):
      neighbour   a pop from the private part returns the entry of a lane that walks the sibling subtree
      deeper      a pop from the private part reads one entry too deep (index sp - lds_depth + 1)
      shallower   ... one entry too shallow
      handover    push keeps entry lds_depth in the LDS part (sp <= lds_depth) while pop looks for it in the private part"""

    def __init__(self, lds_depth=LDS_DEPTH, fault=None):
        self.lds_depth, self.fault = lds_depth, fault
        self.lds = [(0, 0)] * (lds_depth + 1)
        self.spill = [(0, 0)] * (STACK_SIZE - lds_depth + 2)
        self.sp, self.overflow, self.fired = 0, 0, 0

    def push(self, v):
        limit = self.lds_depth + (1 if self.fault == "handover" else 0)
        if self.sp < limit:
            self.lds[self.sp] = v
        elif self.sp < STACK_SIZE:
            self.spill[self.sp - self.lds_depth] = v
        else:
            self.overflow += 1
            return
        self.sp += 1

    def pop(self):
        self.sp -= 1
        if self.sp < self.lds_depth:
            return self.lds[self.sp]
        k = self.sp - self.lds_depth
        if self.fault in ("neighbour", "deeper", "shallower"):
            self.fired += 1
            if self.fault == "neighbour":
                return (self.spill[k][0] + 8, self.spill[k][1])
            return self.spill[k + 1] if self.fault == "deeper" else (self.spill[k - 1] if k else self.lds[self.lds_depth - 1])
        if self.fault == "handover" and k == 0:
            self.fired += 1
        return self.spill[k]


def _safe_inv(v):
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        return (f32(1.0) / np.where(np.abs(v) < 1e-20, np.copysign(f32(1e-20), v), v).astype(f32)).astype(f32)


def _hits(n, o, idir, octinv, tmin, tmax):
    """wide_node_hits in float32, operation by operation (products and sums rounded apart where the device fuses them: a conservative test
    either way, and this walk is held against nothing but its own log)"""
    with np.errstate(all="ignore"):
        scale = np.ldexp(f32(1.0), n["exp"].astype(np.int32) - 127).astype(f32)
        a = (scale * idir).astype(f32)
        b = ((n["origin"].astype(f32) - o) * idir).astype(f32)
        e = ((np.abs(a) * f32(255.0) + np.abs(b)) * f32(4.76837158e-7)).astype(f32)
        qlo = np.stack([n["qlox"], n["qloy"], n["qloz"]], -1).astype(f32)
        qhi = np.stack([n["qhix"], n["qhiy"], n["qhiz"]], -1).astype(f32)
        neg = idir < 0
        tn = (np.where(neg, qhi, qlo) * a + (b - e)).astype(f32)
        tf = (np.where(neg, qlo, qhi) * a + (b + e)).astype(f32)
        tn = np.fmax(np.fmax.reduce(tn, -1), f32(tmin)); tf = np.fmin(np.fmin.reduce(tf, -1), f32(tmax))
        ok = tn <= tf
    hits = 0
    for s in range(8):
        mt = int(n["meta"][s])
        if not mt or not ok[s]:
            continue
        if (mt & 0x1F) >= 24:
            hits |= 1 << (24 + (s ^ octinv))
        else:
            hits |= (mt >> 5) << (mt & 0x1F)
    return hits


def _tri(o, d, v):
    """float64 ray / triangle test in the space of the packets: t or None"""
    e1, e2 = v[1] - v[0], v[2] - v[0]
    p = np.cross(d, e2)
    det = e1 @ p
    if det == 0.0:
        return None
    s = o - v[0]
    u = (s @ p) / det
    q = np.cross(s, e1)
    w = (d @ q) / det
    if u < 0 or w < 0 or u + w > 1:
        return None
    return (e2 @ q) / det


def walk_log(lay, buf, ray, stack=None, max_steps=20000):
    """trace_single<closest> over a traversal copy, with a ModelStack: the log as [n, 4] uint32 rows (code, a, b, sp). A walk that a damaged
    stack sends out of its tree, or that does not end within max_steps, stops where it is: its log then ends without a code 7."""
    inst, nodes, tris, order = bvh_check.split(lay, buf)
    leaf = inst[order]
    stack = stack or ModelStack()
    log = []
    o, tmin, d, tmax = np.asarray(ray[0:3], f32), f32(ray[3]), np.asarray(ray[4:7], f32), f32(ray[7])
    best = (float(tmax), 0xFFFFFFFF, 0)

    def box_ray(ro, rd):
        idir = _safe_inv(rd)
        return ro, idir, (0 if idir[0] < 0 else 4) | (0 if idir[1] < 0 else 2) | (0 if idir[2] < 0 else 1)
    br = box_ray(o, d)
    ro, rd = o.astype(f64), d.astype(f64)
    node_base, tri_base, cur = 0, 0, None
    one = len(inst) == 1
    G, T = ((0, 0), (0, 1)) if one else ((0, 0x80000000), (0, 0))
    put = lambda code, a, b: log.append((code, a & 0xFFFFFFFF, b & 0xFFFFFFFF, stack.sp))
    try:
        while len(log) < max_steps:
            if T[1]:
                i = T[0] + ((T[1] & -T[1]).bit_length() - 1)
                T = (T[0], T[1] & (T[1] - 1))
                if cur is None:
                    it = leaf[i]
                    ntri, x = int(it["triCount"]), int(it["instanceIndex"])
                    if (int(it["mask"]) & 0xFF) and ntri:
                        Wm = it["worldToObject"].reshape(3, 4).astype(f32)
                        ro32 = (Wm[:, :3] @ o + Wm[:, 3]).astype(f32); rd32 = (Wm[:, :3] @ d).astype(f32)
                        ro, rd = ro32.astype(f64), rd32.astype(f64)
                        br = box_ray(ro32, rd32)
                        node_base, tri_base = int(it["nodeBase"]), int(it["triBase"])
                        put(1, x, T[1])
                        stack.push(G); stack.push(T); stack.push(MARKER)
                        cur = x
                        if ntri <= (2 if ntri <= 32 else 1):
                            G, T = (0, 0), (0, (1 << ntri) - 1)
                        else:
                            put(3, 0, 0x80000000)
                            n = nodes[node_base]
                            h = _hits(n, br[0], br[1], br[2], tmin, best[0])
                            G, T = (int(n["childBase"]), (h & 0xFF000000) | int(n["imask"])), (int(n["triBase"]), h & 0x00FFFFFF)
                            put(4, G[1], T[1])
                else:
                    put(2, cur, i)
                    p = tris[tri_base + i]
                    t = _tri(ro, rd, np.stack([p["v0"], p["v1"], p["v2"]]).astype(f64))
                    if t is not None and t > tmin and t < best[0]:
                        best = (t, cur, i)
            elif G[1] > 0x00FFFFFF:
                put(3, G[0], G[1])
                bit = G[1].bit_length() - 1
                G = (G[0], G[1] & ~(1 << bit))
                if G[1] > 0x00FFFFFF:
                    stack.push(G)
                slot = (bit - 24) ^ br[2]
                n = nodes[node_base + G[0] + bin(G[1] & 0xFF & ~(0xFFFFFFFF << slot)).count("1")]
                h = _hits(n, br[0], br[1], br[2], tmin, best[0])
                G, T = (int(n["childBase"]), (h & 0xFF000000) | int(n["imask"])), (int(n["triBase"]), h & 0x00FFFFFF)
                put(4, G[1], T[1])
            elif stack.sp > 0:
                G = stack.pop()
                put(5, G[0], G[1])
                if G == MARKER:
                    if stack.overflow:
                        break
                    T = stack.pop(); G = stack.pop()
                    put(6, G[1], T[1])
                    br = box_ray(o, d); node_base, cur = 0, None
            else:
                put(7, best[1], best[2])
                break
    except IndexError:
        pass
    return np.array(log, np.uint32).reshape(-1, 4)


# ----------------------------------------------------------------------------------------------
# the replay
# ----------------------------------------------------------------------------------------------
def replay(log, one_instance):
    """Runs a model stack along a log. -> dict(max_sp: the largest sp a step logged, blas_levels: the most entries that stood above a
    marker at any step -- the levels of one bottom level, along one path from its root, at which the walk still owed a visit to a hit
    child --, steps, result: (instance, packet) of code 7). Raises AssertionError at the first step the model cannot explain."""
    log = np.asarray(log, np.uint32).reshape(-1, 4)
    stack = []
    G, Ty = ((0, 0), 1) if one_instance else ((0, 0x80000000), 0)        # G.x is None while the log has not shown it yet
    cur, floor, pending6, visited = None, 0, None, None
    out = dict(max_sp=0, blas_levels=0, steps=len(log), result=None)
    for k, (code, a, b, sp) in enumerate(log.tolist()):
        where = f"step {k} (code {code}, a {a:#x}, b {b:#x}, sp {sp})"
        assert out["result"] is None, f"{where}: the log goes on after its end"
        assert code != 0, f"{where}: the log is cut short (no code 7 within its capacity)"
        assert (pending6 is not None) == (code == 6), f"{where}: a popped marker must be followed by the restored top-level state, and only it"
        if code in (1, 2, 3, 4, 7):
            assert sp == len(stack), f"{where}: the model stack holds {len(stack)} entries"
        if code == 1:
            assert cur is None and Ty and b == Ty & (Ty - 1), f"{where}: not the next instance of the group {Ty:#x}"
            stack += [("G", G), ("T", b), ("M", MARKER)]
            cur, floor = a, len(stack)
            G, Ty = (0, 0x80000000), None                                 # a tree of one leaf logs triangles next, any other its root
        elif code == 2:
            assert cur == a, f"{where}: a triangle of instance {a} while the walk is in {cur}"
            if Ty is None:
                G = (0, 0)                                                # the single leaf: its triangle count is not in the log
            else:
                assert Ty, f"{where}: no triangle is left in the group"
                Ty &= Ty - 1
        elif code == 3:
            assert b > 0x00FFFFFF and b == G[1] and (G[0] is None or a == G[0]), f"{where}: the visited group is not the current one {G}"
            assert not Ty, f"{where}: a visit before the triangle group {Ty:#x} is drained"
            rest = b & ~(1 << (b.bit_length() - 1))
            if rest > 0x00FFFFFF:
                stack.append(("N", (a, rest)))
            visited = True
        elif code == 4:
            assert visited, f"{where}: node groups without a visit"
            G, Ty, visited = (None, a), b, None
        elif code == 5:
            assert stack, f"{where}: a pop from an empty model stack"
            assert not Ty and G[1] <= 0x00FFFFFF, f"{where}: a pop while work is left in G {G} / T {Ty}"
            tag, e = stack.pop()
            assert sp == len(stack), f"{where}: the model stack holds {len(stack)} entries after the pop"
            assert tag in "NM" and (a, b) == e, f"{where}: the pop returns ({a:#x}, {b:#x}), the matching push left {tag} {e}"
            if tag == "M":
                pending6 = True
            else:
                G = (a, b)
        elif code == 6:
            (tt, Tp), (tg, Gp) = stack.pop(), stack.pop()
            assert sp == len(stack), f"{where}: the model stack holds {len(stack)} entries after the two pops"
            assert (tt, tg) == ("T", "G") and b == Tp and a == Gp[1], f"{where}: restored ({a:#x}, {b:#x}), parked G {Gp} T {Tp:#x}"
            G, Ty, cur, pending6 = Gp, Tp, None, None
        elif code == 7:
            assert not stack and cur is None, f"{where}: the walk ends with {len(stack)} entries on the model stack"
            out["result"] = (a, b)
        else:
            raise AssertionError(f"{where}: unknown code")
        out["max_sp"] = max(out["max_sp"], sp)
        if cur is not None:
            out["blas_levels"] = max(out["blas_levels"], len(stack) - floor)
    assert out["result"] is not None, "the log has no end (code 7)"
    return out
