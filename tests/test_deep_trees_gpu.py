"""Every traversal stack driven past its LDS part, on trees the device builder makes deep (tests/deepsets.py; the depths and the host
model of the log are checked without a GPU by tests/test_deep_trees_rules.py).

A GroupStack<LDS_DEPTH> (csrc/pt_trace.hpp) keeps its first LDS_DEPTH entries per lane in LDS and the rest in a private array; every
other scene of the suite has a balanced tree on which no lane's sp reaches LDS_DEPTH. Here:

  the tree     the device builds the tree bvhref predicts (19 and 25 bottom levels, 13 + 17 in two levels), before and after a refit
  the witness  pt_debug_trace_ray on 64 rays per scene: max(sp) >= 16 on at least 32 of them, >= 24 in the two-level scene, where the
               fine-end rays enter the deep instance with 9 or 10 entries on the stack, so that G, T and the marker of the transition
               end at the LDS boundary or straddle it. Each log is replayed against a model stack (deepsets.replay)
  the result   walk = device brute force = oracle brute force, ray by ray and bit for bit, closest hit and any hit; frames under every
               schedule equal the oracle's brute-force frame
  refusals     2 (t + b) + 4 = 66 is refused and leaves no top level behind; 64 renders

The flat and the phased walker keep no log. What bounds their sp from below is read off trace_single's log of the same ray:
`blas_levels`, the most entries that stood above an instance's marker at any step. Why that is a bound: inside one instance trace_single
and trace_item (pt_trace2.hpp) run the same loop -- visit_node takes the highest hit bit off G and pushes the rest of G when it still
names a hit child; the triangle group T of the fetched node is drained before the next visit; G is popped when it is exhausted -- with
the same box test, the same slot order (the ray's octant) and the same culling distance, the closest t found so far. trace_closest_flat
resets sp to 0 per item and hands trace_item the scan's verdict with the ray's own tmax as the best t (first batch), and
trace_closest_v2 calls it on top of its top-level entries with h.t, which is tmax while the ray has met nothing: in a scene of ONE
instance both start the item exactly where trace_single stands after its three pushes, so the sequence of visits, pushes and pops is
the same and sp - floor of the item equals trace_single's count of entries above the marker, step by step. (With more instances the
order in which instances are entered differs between the walkers, and with it the culling distance: the bound is claimed for
deep_small and deep_large only, whose frames run the flat walker by default and the phased one under _PHASED.) An entry above the
marker is a level, on the path from the bottom level's root to the node being visited, at which two or more internal children were hit
and one of them is still owed: the top byte of that level's code-4 `a` had two or more bits set."""
import ctypes as C

import numpy as np
import pytest

import bvh_check
import bvhref
import deepsets as D
import isectsets as I
from test_bvh_builder_rules import TLAS, blas_params, leaf_rule

pytestmark = pytest.mark.gpu

f32 = np.float32
BUILT = ("deep_small", "deep_large", "deep_two_level")
GB_KEYS = ("Position", "FlatNormal", "GeometricNormal", "NormalRoughness", "LinearDepth")
# PT_DEBUG_*: default, _LOCKSTEP, _TRAVERSAL_PHASED, _TRAVERSAL_V1, _UNFUSED_ROUNDS, _UNFUSED_ROUNDS | _TRAVERSAL_PHASED, _TRAVERSAL_STATS
SCHEDULES = (0, 0x20, 0x8, 0x4, 0x10, 0x18, 0x1)


class Built:
    """a scene of deepsets on the session's context; closed when the test is over"""

    def __init__(self, gpu, ptamd, name, scene_class=None):
        self.gpu, self.ptamd, self.name = gpu, ptamd, name
        self.soup, self.rays = D.scene(name)
        gpu.set_sharding(0, 1, 16)
        self.g = (scene_class or ptamd.Scene)(gpu, self.soup.scene)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.g.close()


def check_tree(gpu, name, parts, built=None):
    lay, buf = gpu.download_blob()
    bvh_check.check_blob(lay, buf, leaf_rule)
    res = bvhref.check(lay, buf, blas_params, TLAS, parts=parts, accel=gpu.accel_stats(), built=built)
    s = gpu.accel_stats()
    assert (int(s.TopLevelDepth), int(s.MaxBottomLevelDepth)) == D.predicted_depths(name), name
    return lay, buf, res


# ---------------------------------------------------------------------------------------------
# the device builds the predicted tree
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILT)
def test_the_device_builds_the_predicted_tree(gpu, ptamd, name):
    with Built(gpu, ptamd, name):
        lay, buf, res = check_tree(gpu, name, "abcdefg" if name == "deep_small" else "abg")
        if name == "deep_small":
            assert lay.Bytes <= D.BLOB_LDS_MAX, "deep_small is meant to be walked out of LDS"
        else:
            assert lay.Bytes > D.BLOB_LDS_MAX
        if name == "deep_large":
            assert lay.TriangleCount > D.SINGLE_GROUP_LEAVES
        t, b = D.predicted_depths(name)
        print(f"[deep] {name}: top level {t}, bottom level {b} levels as predicted, 2 (t + b) + 4 = {2 * (t + b) + 4}, copy of {lay.Bytes} bytes")


def test_a_refit_keeps_the_deep_tree(gpu, ptamd, pkg):
    """deep_small built for updates, then pt_update_bottom_level with every vertex moved inside its half-cell: the in-place refit keeps
    order, topology and depth; origin, exponents and boxes follow the vertices as they are now"""
    import torch

    class Updatable(ptamd.Scene):
        def _geometry_descs(self, node_index):
            geoms, count, _ = super()._geometry_descs(node_index)
            return geoms, count, 0x8 | 0x1                                   # PREFER_FAST_BUILD | ALLOW_UPDATE

    with Built(gpu, ptamd, "deep_small", Updatable) as b:
        lay, buf, built = check_tree(gpu, "deep_small", "abcdefg")
        mesh, hv, hi = b.soup.scene.geometry[0]
        moved = D.jittered_shells(*D.SPECS["deep_small"]["blas"])
        assert moved.shape == b.soup.nodes[0][0].shape and (moved != b.soup.nodes[0][0]).mean() > 0.9
        v = mesh.vertices.copy()
        v["Position"] = moved.reshape(-1, 3)
        b.g._heap_dev[hv].copy_(torch.from_numpy(v.view(np.uint8).reshape(-1).copy()))
        b.g.UpdateAccelerationStructures(0); gpu.sync()
        lay2, buf2, _ = check_tree(gpu, "deep_small", "abdefg", built=built)
        packets = bvh_check.split(lay2, buf2)[2]
        got = np.stack([packets["v0"], packets["v1"], packets["v2"]], 1)[np.argsort(packets["prim"])]
        assert np.array_equal(got.view(np.uint32), moved.view(np.uint32)), "the refit must have rewritten the packets"


# ---------------------------------------------------------------------------------------------
# the witness: logs of the one-lane walk
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILT)
def test_the_logged_stacks_are_deep_and_replay(gpu, ptamd, name):
    with Built(gpu, ptamd, name) as b:
        idx = D.logged_rays(name)
        assert len(idx) == D.LOGGED
        one = len(b.soup.objects) == 1
        logs = [gpu.trace_ray(b.rays[i]) for i in idx]
        rec = gpu.trace_closest(b.rays[idx])
    res = []
    for i, log, r in zip(idx, logs, rec):
        try:
            res.append(D.replay(log, one))
        except AssertionError as e:
            raise AssertionError(f"{name}, ray {i} {b.rays[i].tolist()}: {e}") from None
        inst, slot = res[-1]["result"]
        assert inst == int(r["Instance"]) and (inst == I.MISS or slot == int(r["Slot"])), (name, i, "code 7 is not trace_closest's record")
    sp = np.array([r["max_sp"] for r in res]); lv = np.array([r["blas_levels"] for r in res])
    entry = sorted({int(s) for log in logs for s in log[log[:, 0] == 1][:, 3]})
    print(f"[deep] {name}: max sp {sp.max()}, >= 16 on {(sp >= 16).sum()} and >= 24 on {(sp >= 24).sum()} of {len(sp)} logs; entries above a marker: "
          f"up to {lv.max()}, >= 12 on {(lv >= 12).sum()}; sp at instance entries {entry}; longest log {max(len(l) for l in logs)} steps")
    # conditions on the inputs (tests/test_deep_trees_rules.py holds the host walk to the same): were they missed, the rays would be wrong
    assert (sp >= 16).sum() >= 32, "fewer than 32 logged rays take the stack of trace_single four entries past its LDS part"
    assert (sp > D.LDS_DEPTH).sum() >= 32
    if name == "deep_two_level":
        assert (sp >= 24).any()
        assert any(D.LDS_DEPTH - 3 < s < D.LDS_DEPTH for s in entry), "no parked top-level state straddles the LDS boundary"
    else:
        # the bound on the flat and the phased walker's sp (module docstring): past kStackLdsFlat and kStackLds2 by four on 32 rays
        assert (lv >= max(D.STACK_LDS_FLAT, D.STACK_LDS_PHASED) + 4).sum() >= 32


def test_trace_ray_refuses_like_the_c_call(gpu, ptamd):
    with pytest.raises(ptamd.PtInvalidArgument):
        gpu.trace_ray(np.zeros(7, f32))
    with pytest.raises(ptamd.PtInvalidArgument):
        gpu.trace_ray(np.zeros(8, f32), log_words=0)
    assert gpu.lib.pt_debug_trace_ray(gpu.handle, None, None, 16) == -1
    with pytest.raises(ptamd.PtError):                                       # no scene is live between the tests: no top level
        gpu.trace_ray(I.rays_of([(0, 0, -1)], [(0, 0, 1)])[0])
    with Built(gpu, ptamd, "deep_small") as b:
        ray = b.rays[D.logged_rays("deep_small")[0]]
        full = gpu.trace_ray(ray)
        assert full[-1, 0] == 7 and 8 < len(full) < 4096
        short = gpu.trace_ray(ray, log_words=4 * 8 + 3)                       # the log ends where its room ends, the walk does not
        assert np.array_equal(short, full[:8])


# ---------------------------------------------------------------------------------------------
# closest hit and any hit, ray by ray, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILT)
def test_walk_equals_brute_force_equals_oracle(gpu, ptamd, oracle, name):
    """every ray: the walk equals the device's brute force in every field, that equals the oracle's brute force bit for bit, and no push
    was refused. The oracle's records of these rays are held against the exact closest hit (isectref.check_closest, 200 per scene) by
    tests/test_deep_trees_rules.py: identical records need no second look here."""
    soup, rays = D.scene(name)
    ref = I.oracle_closest(oracle, soup.scene, rays)
    walk = I.device_records(gpu, ptamd, soup, rays, name, ref)
    hits = float((walk["Instance"] != I.MISS).mean())
    assert hits > 0.1, f"{name}: only {hits:.1%} of the rays hit anything"
    print(f"[deep] {name}: {hits:.1%} of {len(rays)} rays hit, walk = brute force = oracle")


@pytest.mark.parametrize("name", BUILT)
def test_any_hit_equals_the_oracle(gpu, ptamd, oracle, name):
    """pt_trace_visibility with finite intervals. Every geometry here is opaque, so a ray is blocked exactly when some triangle lies
    inside its interval, whatever the order of the walk: the blocked flag must equal the oracle's brute force ray for ray, and an
    unblocked ray's transmittance is (1, 1, 1) in both"""
    import torch
    rays = D.visibility_rays(name)
    assert np.isfinite(rays[:, 7]).all()
    with Built(gpu, ptamd, name) as b:
        want = I.oracle_visibility(oracle, b.soup.scene, rays)
        gpu.reset_counters()
        dr = torch.from_numpy(rays).cuda(); dv = torch.zeros((len(rays), 4), dtype=torch.float32, device="cuda")
        gpu.check(gpu.lib.pt_trace_visibility(gpu.handle, C.c_void_p(dr.data_ptr()), len(rays), C.c_void_p(dv.data_ptr())))
        gpu.sync()
        vis = dv.cpu().numpy()
        assert gpu.counters().StackOverflows == 0
    assert set(np.unique(want[:, 3]).tolist()) == {0.0, 1.0}, "the rays must be blocked in part"
    bad = np.nonzero(vis[:, 3] != want[:, 3])[0]
    assert not len(bad), f"{name}: {len(bad)} rays differ in the blocked flag, first {int(bad[0])}: {rays[bad[0]].tolist()}"
    clear = want[:, 3] == 1
    assert np.array_equal(vis[clear].view(np.uint32), want[clear].view(np.uint32))
    print(f"[deep] {name}: any-hit, {float((want[:, 3] == 0).mean()):.1%} of {len(rays)} rays blocked, equal to the oracle")


# ---------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------
def frame(b, gs, flags=0):
    gpu = b.gpu
    for t in b.r.textures.values():
        t.zero_()
    gpu.set_debug_flags(flags); gpu.reset_counters()
    try:
        b.r.render(gs); gpu.sync()
    finally:
        gpu.set_debug_flags(0)
    return b.ptamd.textures_to_numpy(b.r.textures), gpu.counters()


def assert_frame(out, c, ref, what):
    ref_gb, ref_rays, ref_f32 = ref
    assert c.StackOverflows == 0 and c.PrimaryRays + c.SecondaryRays == ref_rays, what
    for k in GB_KEYS:
        x, y = out[k], ref_gb[k]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (what, k)
    assert np.array_equal(out["RadianceF32"].view(np.uint32), ref_f32.view(np.uint32)), what


@pytest.mark.parametrize("name", BUILT)
def test_frames_under_every_schedule(gpu, ptamd, oracle, pkg, name):
    S, L = pkg.scenes, pkg.layouts
    gs = S.graphics_settings(D.W, D.H, spp=2, bounces=4)
    with Built(gpu, ptamd, name) as b:
        ref = oracle.render(b.soup.scene, gs, accel_mode=0, want_f32=True, layouts=L)
        seen = float(np.isfinite(ref[0]["Position"][..., 3]).mean())
        assert seen > 0.01 and ref[1] > D.W * D.H + 50, f"the camera sees too little: {seen:.1%} of the pixels, {ref[1]} rays"
        b.r = ptamd.Renderer(gpu, b.g, D.W, D.H, with_f32=True)
        for flags in SCHEDULES:
            out, c = frame(b, gs, flags)
            assert_frame(out, c, ref, (name, hex(flags)))
            if flags == 0x1 and name == "deep_large":
                assert c.MaxNodesPerRay > 0, "the streaming kernel did not run"
            if flags == 0x1:
                print(f"[deep] {name}: {seen:.1%} of the pixels hit, {ref[1]} rays, {c.NodesVisited} node visits, longest ray {c.MaxNodesPerRay}")
        out, c = frame(b, gs, 0x2)
        assert c.SecondaryRays > 0 and c.BvhMismatches == 0 and c.StackOverflows == 0, name
        if name == "deep_large":
            try:
                gpu.set_round_chains(3); gpu.set_frames_in_flight(3)
                out, c = frame(b, gs)
                assert_frame(out, c, ref, (name, "3 chains, 3 frames in flight"))
            finally:
                gpu.set_round_chains(0); gpu.set_frames_in_flight(1)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def last_error(gpu):
    return gpu.lib.pt_last_error(gpu.handle).decode()


def cornell_renders(gpu, ptamd, oracle, pkg, what):
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 36
    scene = S.cornell_box(aspect=W / H)
    gs = S.graphics_settings(W, H, spp=2, bounces=4)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    try:
        r = ptamd.Renderer(gpu, g, W, H, with_f32=True)
        gpu.reset_counters(); r.render(gs); gpu.sync()
        out, c = ptamd.textures_to_numpy(r.textures), gpu.counters()
    finally:
        g.close()
    ref_gb, ref_rays, ref_f32 = oracle.render(scene, gs, accel_mode=0, want_f32=True, layouts=L)
    assert c.PrimaryRays + c.SecondaryRays == ref_rays and c.StackOverflows == 0, what
    assert np.array_equal(out["Position"].view(np.uint32), ref_gb["Position"].view(np.uint32)), what
    assert np.array_equal(out["RadianceF32"].view(np.uint32), ref_f32.view(np.uint32)), what


class Deferred:
    """ptamd.Scene whose top-level build is left to the test"""

    @staticmethod
    def of(ptamd):
        class Scene(ptamd.Scene):
            def _build_top_level(self, posed=None):
                if getattr(self, "armed", False):
                    super()._build_top_level(posed)
        return Scene


def test_a_structure_too_deep_is_refused(gpu, ptamd, oracle, pkg):
    """2 (14 + 17) + 4 = 66: the top-level build, or the first call that polls its header, answers PT_ERROR_INVALID_ARGUMENT and names both
    level counts; no top level is left; once the bottom levels are gone a Cornell box renders on the same context"""
    t, bl = D.predicted_depths("too_deep")
    assert 2 * (t + bl) + 4 >= 66
    soup, _ = D.scene("too_deep")
    gpu.set_sharding(0, 1, 16)
    g = Deferred.of(ptamd)(gpu, soup.scene)
    try:
        g.armed = True
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            g._build_top_level()
            gpu.download_blob()                                              # polls the header of the build
        assert "too deep" in str(e.value) and f"top level {t} " in str(e.value) and f"bottom level {bl} " in str(e.value), str(e.value)
        assert last_error(gpu) == str(e.value)
        print(f"[deep] too_deep refused: {e.value}")
        with pytest.raises(ptamd.PtError, match="top-level"):                # NOT_READY: nothing to walk
            gpu.download_blob()
        r = ptamd.Renderer(gpu, g, D.W, D.H, with_f32=True)
        gpu.reset_counters()
        with pytest.raises(ptamd.PtError):
            r.render(pkg.scenes.graphics_settings(D.W, D.H, spp=1, bounces=1)); gpu.sync()
        assert gpu.counters().PrimaryRays == 0, "the refused structure was rendered"
    finally:
        g.close()
    cornell_renders(gpu, ptamd, oracle, pkg, "after the refused scene")


def test_an_update_that_deepens_past_the_bound(gpu, ptamd, oracle, pkg):
    """deep_two_level stands at 64. pt_update_bottom_level with the 19-level mesh in the place of its 17-level one (another triangle
    count: a rebuild under the same id) would make it 68. Under a live top level the update is refused, names both counts, and the old
    tree goes on rendering the same frame. Without a live top level the update goes through -- a bottom level alone is within its own
    bound -- and the top-level build over it is refused and renders nothing; updated back to the first mesh the structure is accepted
    again (the bound counts the LIVE bottom levels, not the deepest the context has ever seen) and renders the frame from before."""
    S, L = pkg.scenes, pkg.layouts
    gs = S.graphics_settings(D.W, D.H, spp=2, bounces=4)
    t, bl = D.predicted_depths("deep_two_level")
    assert D.predicted_depths("deeper_mesh") == (t, bl + 2) and 2 * (t + bl + 2) + 4 > D.STACK_SIZE
    deeper = D.geometry("deeper_mesh")[0][1]
    keep = []

    def update(g, tris):
        v = S.make_vertices(tris.reshape(-1, 3)); ix = S.make_indices(np.arange(tris.size // 3))
        dv, di = ptamd.to_device(v, g.device), ptamd.to_device(ix, g.device)
        keep.extend([dv, di])
        geoms = (ptamd.GeometryDesc * 1)()
        geoms[0].VertexBuffer, geoms[0].VertexCount, geoms[0].VertexStride = dv.data_ptr(), len(v), v.dtype.itemsize
        geoms[0].IndexBuffer, geoms[0].IndexCount, geoms[0].IndexStride = di.data_ptr(), ix.size, ix.dtype.itemsize
        geoms[0].Flags = 1
        gpu.check(gpu.lib.pt_update_bottom_level(gpu.handle, g.blas_ids[1], C.addressof(geoms), 1, 0x4))

    def same(a, b):
        for k in GB_KEYS + ("RadianceF32",):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k

    with Built(gpu, ptamd, "deep_two_level") as b:
        b.r = ptamd.Renderer(gpu, b.g, D.W, D.H, with_f32=True)
        before, c0 = frame(b, gs)
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            update(b.g, deeper)
        assert "too deep" in str(e.value) and f"top level {t} " in str(e.value) and f"bottom level {bl + 2} " in str(e.value), str(e.value)
        print(f"[deep] update refused: {e.value}")
        s = gpu.accel_stats()
        assert (int(s.TopLevelDepth), int(s.MaxBottomLevelDepth)) == (t, bl)
        again, c1 = frame(b, gs)                                             # the old tree, the old top level
        assert c1.StackOverflows == 0 and c1.PrimaryRays + c1.SecondaryRays == c0.PrimaryRays + c0.SecondaryRays
        same(before, again)

    soup, _ = D.scene("deep_two_level")
    gpu.set_sharding(0, 1, 16)
    g = Deferred.of(ptamd)(gpu, soup.scene)
    try:
        update(g, deeper)                                                    # no top level is live: accepted
        g.armed = True
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            g._build_top_level()
            gpu.download_blob()
        assert f"top level {t} " in str(e.value) and f"bottom level {bl + 2} " in str(e.value), str(e.value)
        b.g, b.r = g, ptamd.Renderer(gpu, g, D.W, D.H, with_f32=True)
        gpu.reset_counters()
        with pytest.raises(ptamd.PtError):
            b.r.render(gs); gpu.sync()
        assert gpu.counters().PrimaryRays == 0
        update(g, soup.nodes[1][0])
        g._build_top_level()
        s = gpu.accel_stats()                                                # polls the header: accepted
        assert (int(s.TopLevelDepth), int(s.MaxBottomLevelDepth)) == (t, bl)
        after, c2 = frame(b, gs)
        assert c2.StackOverflows == 0 and c2.PrimaryRays + c2.SecondaryRays == c0.PrimaryRays + c0.SecondaryRays
        same(before, after)
    finally:
        g.close()
