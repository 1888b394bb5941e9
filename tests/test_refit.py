"""The dynamic-scene path at the sizes where it can go wrong: pt_skin_mesh, then pt_update_bottom_level as an in-place refit
(k_tri_setup through slotOfPrim, k_leaves, k_refit without cost tables, k_requantise), then pt_build_top_level.

tests/test_skinning.py refits 96 triangles: one k_refit workgroup, so neither the hand-off of boxes between workgroups nor the state
that must survive from one refit to the next (the arrival counters k_refit resets for its next launch) is ever at work there, and no
test looks at a refitted structure or at a triangle packet after a refit. Here, per triangle count (why each: SIZES), a skinned strip
of tests/skinref.py goes through rest -> scale -> far -> huge -> flat -> rigid -> rest, and after EVERY refit
  1. bvh_check.check_blob passes on the downloaded traversal copy (slot boxes contain the deformed triangles, every triangle is
     reached once, instance world boxes contain the transformed vertices),
  2. bvh_check.check_packets passes (every packet holds its triangle's vertices as they are on the device now, bit for bit, beside
     its row of vertex indices: a refit that rewrote boxes but left stale packets, or wrote packets into the wrong slots, passes
     check_blob),
  3. accel_stats() shows node bytes, depths and NormalRecords as after the build, and the frame has no stack overflow,
  4. the frame equals the oracle's brute-force frame (accel_mode = 0) over the host-skinned mesh: G-buffer, RadianceF32, ray count.
     The oracle renders the `flat` pose like any other (it rejects nothing), so `flat` is not exempt,
  5. the frame rendered again after CreateAccelerationStructures() -- a fresh build from the current vertices -- is bit-identical,
  6. and one frame per size under PT_DEBUG_BRUTE_FORCE has BvhMismatches == 0.
Then: history independence (a chain of refits ends in the same tree, boxes and packets as one refit of a fresh scene), the rebuild
fall-back of pt_update_bottom_level, and frames enqueued with no host wait between skin, update and render."""
import numpy as np
import pytest

import bvh_check
import skinref

pytestmark = pytest.mark.gpu

W, H = 64, 36
JOINTS = 6
SKINNED_NODE = 2
GB_KEYS = ("Position", "FlatNormal", "GeometricNormal", "NormalRoughness", "MotionVector", "LinearDepth")
SEQUENCE = ("rest", "scale", "far", "huge", "flat", "rigid", "rest")
# triangle count(s) of the skinned mesh node -> what it exercises
SIZES = {
    (2,): "a single leaf, no nodes, root bounds only",
    (31,): "two triangles per leaf, an odd last leaf",
    (33,): "the first size with one triangle per leaf",
    (264,): "two k_refit workgroups; the instance box is still taken from the vertices",
    (1320,): "above kExactBoxTriangles: the instance box is decoded from refitted child boxes",
    (4164,): "above kSingleGroupCollapseLeaves: slotRefs were written by the level-by-level collapse",
    (264, 33): "two skinned geometries in one node, updated in a single call",
}


def leaf_rule(n):            # pt_trace.hpp blas_leaf_tris
    return 2 if n <= 32 else 1


def pose_of(kind, seed):
    return skinref.rest_pose(JOINTS) if kind == "rest" else skinref.poses(JOINTS, kind, seed)


def strips(sizes, seed):
    out = []
    for k, n in enumerate(sizes):
        m = skinref.skinned_strip(n, JOINTS, seed + k)
        for a in (m.vertices, m.skeletal_vertices):                  # side by side, not through one another
            a["Position"][:, 0] += np.float32(0.35 * k)
        out.append(m)
    return out


def oracle_skin(oracle, mesh, transforms):
    tr = np.ascontiguousarray(transforms, np.float32)
    oracle.lib().or_skin_mesh(mesh.skeletal_vertices.ctypes.data, tr.ctypes.data, mesh.vertices.ctypes.data,
                              mesh.motion_vectors.ctypes.data, len(mesh.vertices))


class Rig:
    """scenes.dynamic_scene() with skinned strips in its third mesh node, on the device and (skinned by the oracle) on the host."""

    def __init__(self, gpu, ptamd, oracle, pkg, sizes, seed=5, scene_class=None, **scene_args):
        self.gpu, self.ptamd, self.oracle, self.S, self.L = gpu, ptamd, oracle, pkg.scenes, pkg.layouts
        self.meshes = strips(sizes, seed)
        self.scene = self.S.dynamic_scene(aspect=W / H, meshes=self.meshes)
        gpu.set_sharding(0, 1, 16)
        self.g = (scene_class or ptamd.Scene)(gpu, self.scene, **scene_args)
        self.r = ptamd.Renderer(gpu, self.g, W, H, with_f32=True)

    def close(self):
        self.g.close()

    def skin(self, transforms, host=True):
        for m in self.meshes:
            self.g.SkinSkeletalMeshes(m, transforms)
            if host:
                oracle_skin(self.oracle, m, transforms)

    def pose(self, transforms):
        self.skin(transforms)
        self.g.UpdateAccelerationStructures(SKINNED_NODE)
        self.gpu.sync()

    def settings(self, frame_index):
        return self.S.graphics_settings(W, H, spp=2, bounces=4, frame_index=frame_index)

    def frame(self, frame_index, debug_flags=0):
        for t in self.r.textures.values():
            t.zero_()           # miss pixels keep whatever the textures held; the oracle starts from zeros
        self.gpu.set_debug_flags(debug_flags)
        try:
            self.gpu.reset_counters(); self.r.render(self.settings(frame_index)); self.gpu.sync()
        finally:
            self.gpu.set_debug_flags(0)
        return self.ptamd.textures_to_numpy(self.r.textures), self.gpu.counters()

    def device_vertices(self, mesh):
        hv = next(h for m, h, _ in self.scene.geometry if m is mesh)
        return self.g.download(hv, np.uint8).view(self.L.VERTEX)

    def geometries(self):
        """per instance, for bvh_check.check_packets: the static nodes from the host arrays, the skinned node from the device"""
        out = []
        for ro in self.scene.objects:
            node = self.scene.nodes[ro.node]
            out.append([((self.device_vertices(m) if ro.node == SKINNED_NODE else m.vertices)["Position"], m.indices) for m in node.meshes])
        return out

    def check_structure(self):
        lay, buf = self.gpu.download_blob()
        st = bvh_check.check_blob(lay, buf, leaf_rule)
        bvh_check.check_packets(lay, buf, self.geometries())
        return lay, buf, st

    def check_against_oracle(self, out, c, frame_index, what):
        for m in self.meshes:                                        # the device skinned what the host skinned
            assert np.array_equal(self.device_vertices(m).view(np.uint8), m.vertices.view(np.uint8)), what
        ref_gb, ref_rays, ref_f32 = self.oracle.render(self.scene, self.settings(frame_index), accel_mode=0, want_f32=True, layouts=self.L)
        for k in GB_KEYS:
            a, b = out[k], ref_gb[k]
            if a.dtype.kind == "f":
                a, b = a.view(np.uint32), b.view(np.uint32)
            assert np.array_equal(a, b), (what, k)
        assert c.PrimaryRays + c.SecondaryRays == ref_rays, what
        assert np.array_equal(out["RadianceF32"].view(np.uint32), ref_f32.view(np.uint32)), what


def stats_key(s):
    return (s.NodeBytes, s.TriangleBytes, s.MaxBottomLevelDepth, s.TopLevelDepth, s.NormalRecords, s.InstanceCount, s.TriangleCount)


def same_frame(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (what, k)


@pytest.mark.parametrize("sizes", list(SIZES), ids=["+".join(map(str, s)) for s in SIZES])
def test_refit_through_a_pose_sequence(gpu, ptamd, oracle, pkg, sizes):
    rig = Rig(gpu, ptamd, oracle, pkg, sizes)
    try:
        assert [m.indices.size // 3 for m in rig.meshes] == list(sizes)
        rig.check_structure()
        rig.frame(0)                                                 # NormalRecords is decided by the first frame over a binding
        built = stats_key(gpu.accel_stats())
        for step, kind in enumerate(SEQUENCE):
            what = (sizes, step, kind)
            rig.pose(pose_of(kind, seed=100 + step))
            rig.check_structure()                                    # 1, 2
            out, c = rig.frame(step)
            assert stats_key(gpu.accel_stats()) == built, what       # 3: a refit moves boxes and packets, nothing else
            assert c.StackOverflows == 0, what
            rig.check_against_oracle(out, c, step, what)             # 4
            if kind == "scale":                                      # 6
                _, cb = rig.frame(step, debug_flags=2)
                assert cb.SecondaryRays > 0 and cb.BvhMismatches == 0 and cb.StackOverflows == 0, what
            rig.g.CreateAccelerationStructures()                     # 5: topology must not show in the image
            again, c2 = rig.frame(step)
            same_frame(out, again, what)
            assert c2.PrimaryRays + c2.SecondaryRays == c.PrimaryRays + c.SecondaryRays, what
            built = stats_key(gpu.accel_stats())
    finally:
        rig.close()


@pytest.mark.parametrize("sizes", [(264,), (4164,)], ids=["264", "4164"])
def test_refit_does_not_depend_on_history(gpu, ptamd, oracle, pkg, sizes):
    """Scene A: rest -> scale -> huge -> rigid by three refits. Scene B: a new scene from the rest-pose data, refitted straight to the
    same rigid pose. Instance records, the skinned bottom level's nodes and its packets must be equal field for field (compared in
    depth-first slot order: where the builder's allocation counters put a node is not structure). A box that only ever grows, an
    arrival counter left non-zero by the refit before, a box read stale across workgroups: each shows here. Then A goes back to the rest
    pose and must render the frame of a freshly built rest scene."""
    last = pose_of("rigid", 203)
    a = Rig(gpu, ptamd, oracle, pkg, sizes)
    try:
        for k, kind in enumerate(("scale", "huge")):
            a.pose(pose_of(kind, 201 + k))
        a.pose(last)
        lay, buf, _ = a.check_structure()
        inst_a = bvh_check.split(lay, buf)[0].copy()
        nodes_a, tris_a = bvh_check.canonical_blas(lay, buf, SKINNED_NODE, leaf_rule)
        for _ in range(2):                                           # twice: the second time nothing moves, motion vectors are zero
            a.pose(pose_of("rest", 0))
        a.check_structure()
        rest_a, _ = a.frame(9)
    finally:
        a.close()
    b = Rig(gpu, ptamd, oracle, pkg, sizes)
    try:
        b.pose(last)
        lay, buf, _ = b.check_structure()
        inst_b = bvh_check.split(lay, buf)[0].copy()
        nodes_b, tris_b = bvh_check.canonical_blas(lay, buf, SKINNED_NODE, leaf_rule)
    finally:
        b.close()
    bvh_check.assert_records_equal(inst_a, inst_b, "instance records")
    bvh_check.assert_records_equal(nodes_a, nodes_b, "nodes of the skinned bottom level")
    bvh_check.assert_records_equal(tris_a, tris_b, "packets of the skinned bottom level")
    fresh = Rig(gpu, ptamd, oracle, pkg, sizes)
    try:
        for _ in range(2):
            fresh.pose(pose_of("rest", 0))
        rest_f, _ = fresh.frame(9)
    finally:
        fresh.close()
    same_frame(rest_a, rest_f, "back at the rest pose")


def test_checkers_notice_a_damaged_structure(gpu, ptamd, oracle, pkg):
    """The checkers' self-test on a downloaded blob that numpy alters ON THE HOST (nothing runs on a damaged structure): a slot box
    shrunk, a packet vertex put back to its rest-pose value, two packets swapped. Each must raise."""
    rig = Rig(gpu, ptamd, oracle, pkg, (264,))
    try:
        rest = rig.meshes[0].vertices["Position"].copy()
        rig.pose(pose_of("scale", 301))
        lay, buf, _ = rig.check_structure()
        geoms = rig.geometries()
    finally:
        rig.close()
    inst, nodes, tris, _ = bvh_check.split(lay, buf)
    nb, tb, tc = (int(inst[SKINNED_NODE][k]) for k in ("nodeBase", "triBase", "triCount"))
    assert tc == 264

    def damaged():
        d = buf.copy()
        return d, bvh_check.split(lay, d)

    # one qhi byte lowered: the first leaf slot of the bottom level that is at least two quanta wide, on its widest axis, down to its qlo
    d, (_, dn, _, _) = damaged()
    end = min([int(x) for x in inst["nodeBase"] if int(x) > nb] + [int(lay.NodeCount)])

    def width(n, s, a):
        return int(dn[n]["qhi" + a][s]) - int(dn[n]["qlo" + a][s])
    n, s = next((n, s) for n in range(nb, end) for s in range(8)
                if dn[n]["meta"][s] and (dn[n]["meta"][s] & 0x1F) < 24 and max(width(n, s, a) for a in "xyz") >= 2)
    axis = max("xyz", key=lambda a: width(n, s, a))
    dn["qhi" + axis][n, s] = dn[n]["qlo" + axis][s]
    with pytest.raises(AssertionError, match="stick out"):
        bvh_check.check_blob(lay, d, leaf_rule)
    bvh_check.check_packets(lay, d, geoms)                            # (the packets are as they were)
    # one packet vertex replaced by its rest-pose value
    d, (_, _, dt, _) = damaged()
    prim = int(dt[tb + 7]["prim"])
    vi = int(rig.meshes[0].indices[3 * prim + 1])
    assert not np.array_equal(rest[vi], geoms[SKINNED_NODE][0][0][vi])
    dt["v1"][tb + 7] = rest[vi]
    with pytest.raises(AssertionError, match="does not hold"):
        bvh_check.check_packets(lay, d, geoms)
    # two packets swapped: each still holds a triangle of the mesh and every (geometry, primitive) occurs once, but not where the boxes
    # are, and not beside its row of vertex indices
    d, (_, _, dt, _) = damaged()
    centre = (dt["v0"][tb:tb + tc] + dt["v1"][tb:tb + tc] + dt["v2"][tb:tb + tc]) / 3.0
    i = 0
    j = int(np.argmax(np.abs(centre - centre[i]).max(1)))
    x, y = dt[tb + i].copy(), dt[tb + j].copy()
    dt[tb + i], dt[tb + j] = y, x
    with pytest.raises(AssertionError, match="carries the vertex indices"):
        bvh_check.check_packets(lay, d, geoms)
    with pytest.raises(AssertionError, match="stick out"):
        bvh_check.check_blob(lay, d, leaf_rule)


def flag_scene(ptamd):
    class FlagScene(ptamd.Scene):
        """a Scene whose skinned node is built and updated with the build flags the test chooses (None: ALLOW_UPDATE | PREFER_FAST_BUILD)"""
        node_flags = None

        def __init__(self, ctx, scene, node_flags=None):
            self.node_flags = node_flags
            super().__init__(ctx, scene)

        def _geometry_descs(self, node_index):
            geoms, count, flags = super()._geometry_descs(node_index)
            if node_index == SKINNED_NODE and self.node_flags is not None:
                flags = self.node_flags
            return geoms, count, flags
    return FlagScene


PREFER_FAST_TRACE, ALLOW_UPDATE, PREFER_FAST_BUILD = 0x4, 0x1, 0x8


def test_update_falls_back_to_a_rebuild(gpu, ptamd, oracle, pkg):
    """pt_update_bottom_level on a structure that cannot be refitted -- built without ALLOW_UPDATE, or updated with another triangle
    count -- rebuilds it under its id: PT_OK, a sound structure over the new vertices and counts, the oracle's frame. Once the structure
    is updatable and the counts agree, the next update is a refit: the node bytes stay."""
    # built without ALLOW_UPDATE
    rig = Rig(gpu, ptamd, oracle, pkg, (264,), scene_class=flag_scene(ptamd), node_flags=PREFER_FAST_TRACE)
    try:
        rig.pose(pose_of("scale", 401))                               # no flag: rebuilt, still not updatable
        rig.check_structure()
        out, c = rig.frame(1)
        rig.check_against_oracle(out, c, 1, "update without ALLOW_UPDATE")
        rig.g.node_flags = ALLOW_UPDATE | PREFER_FAST_BUILD
        rig.pose(pose_of("rigid", 402))                               # rebuilt once more, now for updates
        rig.check_structure()
        out, c = rig.frame(2)
        rig.check_against_oracle(out, c, 2, "update that turns ALLOW_UPDATE on")
        before = stats_key(gpu.accel_stats())
        rig.pose(pose_of("scale", 403))                               # a refit
        rig.check_structure()
        out, c = rig.frame(3)
        assert stats_key(gpu.accel_stats()) == before
        rig.check_against_oracle(out, c, 3, "refit after the fall-back")
    finally:
        rig.close()
    # built for updates, then updated with one geometry three indices shorter
    rig = Rig(gpu, ptamd, oracle, pkg, (264, 33))
    try:
        built = gpu.accel_stats()
        m = rig.meshes[0]
        m.indices = m.indices[:-3].copy()                             # host: the oracle and the geometry descs read the count from here
        rig.pose(pose_of("scale", 404))
        lay, buf, _ = rig.check_structure()
        assert int(bvh_check.split(lay, buf)[0][SKINNED_NODE]["triCount"]) == 263 + 33
        assert gpu.accel_stats().TriangleCount == built.TriangleCount - 1
        out, c = rig.frame(1)
        rig.check_against_oracle(out, c, 1, "update with a shorter index buffer")
        before = stats_key(gpu.accel_stats())
        rig.pose(pose_of("rigid", 405))                               # a refit of the 263 + 33 triangles
        rig.check_structure()
        out, c = rig.frame(2)
        assert stats_key(gpu.accel_stats()) == before
        rig.check_against_oracle(out, c, 2, "refit after the change of counts")
    finally:
        rig.close()


def test_frames_enqueued_without_synchronisation(ptamd, oracle, pkg):
    """Twelve poses back to back on a caller's stream with NO host wait: skin, update, render, then a stream-ordered clone of Position
    and RadianceF32. Every clone must be the frame rendered for that pose with a sync after every step: a refit or a top-level rebuild
    overtaking a frame still in flight (or the other way round) shows in the image."""
    import torch
    S = pkg.scenes
    poses = [pose_of(("scale", "rigid", "mirror")[k % 3], 500 + k) for k in range(12)]     # more frames than the staging rings have slots
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx = ptamd.DeviceContext(0, stream=stream.cuda_stream)
        try:
            rig = Rig(ctx, ptamd, oracle, pkg, (264,))
            settings = [S.graphics_settings(W, H, spp=2, bounces=4, frame_index=k) for k in range(len(poses))]

            def run(wait):
                rig.pose(pose_of("rest", 0))                          # every run starts from the same vertices
                for t in rig.r.textures.values():
                    t.zero_()                                         # and textures: a miss pixel keeps what the frame before left
                clones = []
                for k, tr in enumerate(poses):
                    rig.skin(tr, host=False)
                    if wait: ctx.sync()
                    rig.g.UpdateAccelerationStructures(SKINNED_NODE)
                    if wait: ctx.sync()
                    rig.r.render(settings[k])
                    if wait: ctx.sync()
                    clones.append((rig.r.textures["Position"].clone(), rig.r.textures["RadianceF32"].clone()))   # stream-ordered behind the frame
                ctx.sync()
                return [(p.cpu().numpy().view(np.uint32), f.cpu().numpy().view(np.uint32)) for p, f in clones]

            want = run(True)
            assert any(not np.array_equal(want[0][0], w[0]) for w in want[1:])             # the poses do show in the image
            for inflight, chains in ((1, 1), (3, 3)):
                try:
                    ctx.set_frames_in_flight(inflight); ctx.set_round_chains(chains)
                    got = run(False)
                finally:
                    ctx.set_frames_in_flight(1); ctx.set_round_chains(0)
                for k in range(len(poses)):
                    assert np.array_equal(got[k][0], want[k][0]), (inflight, chains, k, "Position")
                    assert np.array_equal(got[k][1], want[k][1]), (inflight, chains, k, "RadianceF32")
            rig.close()
        finally:
            ctx.close()
