"""Animation playback on the device (include/ptamd.h pt_anim_*, pt_build_top_level_posed; DESIGN.md section 1, "Animation"), -m gpu.

The pose against tests/animref.py's float64 restatement within its running error bound, and the hand-offs bit for bit against the paths the
library already had: skinning with host matrices (Scene.SkinSkeletalMeshes) and the top level over host descriptors (pt_build_top_level).
Everything renders 64 x 64 at 1 spp."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 64
UNFUSED, LOCKSTEP = 0x10, 0x20
NO_NODE = 0xFFFFFFFF


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref():
    return _module("animref")


@pytest.fixture(scope="module")
def sets():
    return _module("animsets")


class Stage:
    """a context of its own with the animated scene on it: scene, renderer, animation"""

    def __init__(self, ptamd, pkg, scene=None, animate=True):
        self.ptamd, self.S = ptamd, pkg.scenes
        self.ctx = ptamd.DeviceContext(0)
        self.ctx.set_sharding(0, 1, 16)
        self.desc = scene if scene is not None else pkg.scenes.animated_scene(aspect=W / H)
        self.scene = ptamd.Scene(self.ctx, self.desc)
        self.renderer = ptamd.Renderer(self.ctx, self.scene, W, H, with_f32=True)
        self.animation = ptamd.Animation(self.ctx, self.desc.animations) if animate else None

    def frame(self, flags=0, frame_index=0):
        """every texture of one frame as bytes, and the ray counts"""
        gs = self.S.graphics_settings(W, H, spp=1, bounces=3, frame_index=frame_index)
        for t in self.renderer.textures.values():
            t.zero_()
        try:
            self.ctx.set_debug_flags(flags)
            self.ctx.reset_counters()
            self.renderer.render(gs)
            self.ctx.sync()
        finally:
            self.ctx.set_debug_flags(0)
        c = self.ctx.counters()
        out = {k: v.copy() for k, v in self.ptamd.textures_to_numpy(self.renderer.textures).items()}
        out["rays"] = np.array([c.PrimaryRays, c.SecondaryRays], np.uint64)
        return out

    def close(self):
        if self.animation is not None:
            self.animation.close()
        self.scene.close()
        self.ctx.close()


def _same_frame(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _instance_data(stage, L):
    stage.ctx.sync()
    n = len(stage.desc.objects)
    return stage.scene.instance_data.cpu().numpy()[:n * L.INSTANCE_DATA.itemsize].view(L.INSTANCE_DATA).copy()


# ------------------------------------------------------------------------------------------------------------------------------ arithmetic
def _slerp_cases(rig, states):
    """every (q0, q1, t) a rotation channel of the parity set interpolates, as the device forms them"""
    q0, q1, ts = [], [], []
    for pair in states:
        for clip, time in pair:
            for n in range(len(rig.parents)):
                first, count = (int(v) for v in rig.channels[clip, n, 1])
                kt = rig.key_times[first:first + count].astype(np.float64)
                if count < 2 or time < kt[0] or time >= kt[-1]:
                    continue
                i = int(np.searchsorted(kt, time, side="right")) - 1
                q0.append(rig.key_values[first + i]); q1.append(rig.key_values[first + i + 1])
                ts.append(np.float32((time - kt[i]) / (kt[i + 1] - kt[i])))
    return np.array(q0, np.float32), np.array(q1, np.float32), np.array(ts, np.float32)


def test_device_sqrt_atan2_sin_error_is_within_the_constants_of_the_reference(gpu, ptamd, pkg, ref, sets):
    """The ulp error of the device's sqrtf / atan2f / sinf cannot be derived from the format: measured here against float64 on the slerp
    cases of the parity set (inputs as the device had them), and animref's constants must be at least twice the measured maximum.
    Measured on gfx950: see animref.MEASURED."""
    rig = sets.parity_rig(pkg.scenes)
    q0, q1, t = _slerp_cases(rig, sets.STATES)
    extra = np.linspace(0.0, 1.0, 41, dtype=np.float32)                  # and a sweep of t over each distinct key pair
    pairs = np.unique(np.concatenate([q0, q1], 1), axis=0)
    q0 = np.concatenate([q0, np.repeat(pairs[:, :4], len(extra), 0)]); q1 = np.concatenate([q1, np.repeat(pairs[:, 4:], len(extra), 0)])
    t = np.concatenate([t, np.tile(extra, len(pairs))])
    out = ptamd.debug_slerp(gpu, q0, q1, t).astype(np.float64)
    c, x, s, w, a0, a1, n0, n1 = (out[:, 4 + k] for k in range(8))
    on = s > 0                                                           # the slerp branch
    assert on.sum() >= 100 and (~on).sum() >= 10
    rel = lambda got, want: float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) / ref.U
    measured = {"sqrtf": rel(s[on], np.sqrt(x[on])), "atan2f": rel(w[on], np.arctan2(s[on], c[on])),
                "sinf": max(rel(n0[on][a0[on] != 0], np.sin(a0[on][a0[on] != 0])), rel(n1[on][a1[on] != 0], np.sin(a1[on][a1[on] != 0])))}
    print("measured relative error in units of u = 2^-24:", {k: round(v, 3) for k, v in measured.items()})
    assert 2.0 * measured["sqrtf"] <= ref.K_SQRT and 2.0 * measured["atan2f"] <= ref.K_ATAN2 and 2.0 * measured["sinf"] <= ref.K_SIN, measured
    worst = 0.0
    for k in range(len(t)):                                              # and the slerp itself within the reference's bound
        q, _ = ref.slerp(ref.Bd(q0[k].astype(np.float64)), ref.Bd(q1[k].astype(np.float64)), ref.Bd(float(t[k])))
        d = np.abs(out[k, :4] - q.v)
        assert np.all(d <= 2.0 * q.e), (k, d, q.e)
        worst = max(worst, float(np.max(d / np.maximum(q.e, 1e-300))))
    print("slerp: largest error / bound =", round(worst, 3))


def test_pose_parity_two_objects_sharing_a_rig_in_one_call(ptamd, pkg, ref, sets):
    S, L = pkg.scenes, pkg.layouts
    import torch
    ctx = ptamd.DeviceContext(0)
    try:
        objs = sets.parity_objects(S)
        inst = torch.zeros(4 * L.INSTANCE_DATA.itemsize, dtype=torch.uint8, device=torch.device("cuda", 0))
        ctx.check(ctx.lib.pt_set_instance_data(ctx.handle, C.c_void_p(inst.data_ptr()), 4))
        anim = ptamd.Animation(ctx, objs)
        worst = 0.0

        def within(got, want, what):
            nonlocal worst
            d = np.abs(got.astype(np.float64) - want.v)
            assert np.all(d <= 2.0 * want.e + 0.0), (what, d.max(), want.e.max())
            worst = max(worst, float(np.max(d / np.maximum(want.e, 1e-300))))

        for pair in sets.STATES:
            for i, (clip, time) in enumerate(pair):
                anim.SetSelectedIndex(i, clip)
                anim.times[i] = time                                     # (SetTime clamps; the states include times beyond the duration)
            anim.Evaluate(inst)
            got = []
            for i, (clip, time) in enumerate(pair):
                g = anim.download_globals(i)
                want = ref.pose(objs[i].rig, clip, time)
                assert len(g) == len(want) == 7
                for s in objs[i].skins:
                    if int(s.mesh_node) != NO_NODE:
                        assert ref.condition(want[int(s.mesh_node)].v) <= 1e3       # what the neglected second-order terms rest on
                for n in range(7):
                    within(g[n], want[n], ("global", pair, i, n))
                sk = [anim.download_skeletal(i, k) for k in range(len(objs[i].skins))]
                for k in range(len(objs[i].skins)):
                    for j, m in enumerate(ref.skeletal_transforms(objs[i], want, k)):
                        if m is None:
                            assert not sk[k][j].any(), "a joint / mesh node without a rig node keeps its matrix"
                        else:
                            within(sk[k][j], m, ("skeletal", pair, i, k, j))
                data = inst.cpu().numpy().view(L.INSTANCE_DATA)
                for b, m in enumerate(ref.instance_transforms(objs[i], want)):
                    within(data[int(objs[i].binding_instances[b])]["ObjectToWorld"], m, ("instance", pair, i, b))
                got.append((g, sk, data["ObjectToWorld"].copy()))
            anim.Evaluate(inst)                                          # the same call again: the same bits
            for i in range(2):
                assert np.array_equal(anim.download_globals(i).view(np.uint32), got[i][0].view(np.uint32))
                for k in range(len(objs[i].skins)):
                    assert np.array_equal(anim.download_skeletal(i, k).view(np.uint32), got[i][1][k].view(np.uint32))
            assert np.array_equal(inst.cpu().numpy().view(L.INSTANCE_DATA)["ObjectToWorld"].view(np.uint32), got[1][2].view(np.uint32))
        print("pose parity: largest error / bound =", round(worst, 3))
        assert worst > 1e-3, "the bound is never approached: it would hide a wrong pose"
        anim.close()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------- hand-offs
def test_hand_off_to_skinning_is_bit_exact(ptamd, pkg):
    """Animate skins from the joint matrices where the pose left them; the vertex and motion-vector buffers equal, bit for bit, those of
    the existing SkinSkeletalMeshes(mesh, host matrices) fed the downloaded matrices, on a second copy of the scene."""
    a, b = Stage(ptamd, pkg), Stage(ptamd, pkg, animate=False)
    try:
        bar_a, bar_b = a.desc.nodes[2].meshes[0], b.desc.nodes[2].meshes[0]
        hv = next(h for m, h, _ in a.desc.geometry if m is bar_a); hm = int(a.desc._motion_heap[id(bar_a)])
        rest = a.scene.download(hv, np.uint8).copy()
        for clip, time in ((0, 0.37), (0, 0.8), (1, 1.1)):
            a.animation.SetSelectedIndex(0, clip); a.animation.SetTime(time)
            a.scene.Animate(a.animation)
            matrices = a.animation.download_skeletal(0, 0)
            assert matrices.shape == (2, 3, 4)
            if clip == 0:                                                # clip 0 bends the column at joint1: the two joints' matrices differ
                assert not np.array_equal(matrices[0], matrices[1])
            b.scene.SkinSkeletalMeshes(bar_b, matrices)
            a.ctx.sync(); b.ctx.sync()
            va, vb = a.scene.download(hv, np.uint8), b.scene.download(hv, np.uint8)
            assert np.array_equal(va, vb), (clip, time)
            assert np.array_equal(a.scene.download(hm, np.uint16), b.scene.download(hm, np.uint16)), (clip, time)
            assert not np.array_equal(va, rest)
            sk = bar_a.skeletal_vertices["Weights"]
            assert (sk[:, 0] > 0.9).any() and (sk[:, 1] > 0.9).any()                                 # the column rebinds both joints
    finally:
        a.close(); b.close()


def _host_posed_copy(ptamd, pkg, a, L):
    """a second copy of the scene, brought to stage a's pose through the paths the library had: host joint matrices, host descriptors"""
    b = Stage(ptamd, pkg, animate=False)
    data = _instance_data(a, L)
    b.scene.instance_data[:data.nbytes].copy_(__import__("torch").from_numpy(data.view(np.uint8).copy()))
    bar_b = b.desc.nodes[2].meshes[0]
    b.scene.SkinSkeletalMeshes(bar_b, a.animation.download_skeletal(0, 0))
    for i in range(len(b.desc.objects)):
        b.scene._descs[i].Transform = (C.c_float * 12)(*data[i]["ObjectToWorld"].reshape(12).tolist())
    b.scene.UpdateAccelerationStructures(2)                              # refit + pt_build_top_level over the host descriptors
    return b


def test_posed_top_level_equals_the_host_descriptors_byte_for_byte(ptamd, pkg):
    L = pkg.layouts
    a = Stage(ptamd, pkg)
    b = None
    try:
        a.animation.SetTime(0.37)
        a.scene.Animate(a.animation)
        b = _host_posed_copy(ptamd, pkg, a, L)
        moved = _instance_data(a, L)["ObjectToWorld"]
        assert not np.array_equal(moved[3], a.desc.instance_data["ObjectToWorld"][3])               # the pose did move the rigid box
        for flags in (0, UNFUSED, LOCKSTEP):
            _same_frame(a.frame(flags), b.frame(flags), flags)
        # from_device all zero: the call is pt_build_top_level
        zeros = np.zeros(len(a.desc.objects), np.uint8)
        for i in range(len(a.desc.objects)):
            a.scene._descs[i].Transform = (C.c_float * 12)(*moved[i].reshape(12).tolist())
        a.scene._build_top_level(posed=zeros)
        plain = a.frame()
        _same_frame(plain, b.frame(), "from_device all zero")
        a.scene._build_top_level()
        _same_frame(plain, a.frame(), "pt_build_top_level")
        a.scene._build_top_level(posed=a.animation.from_device(len(a.desc.objects)))
        _same_frame(plain, a.frame(), "posed again")
    finally:
        a.close()
        if b is not None:
            b.close()


def test_motion_previous_transform_and_motion_vectors(ptamd, pkg):
    """Two consecutive poses: the moving rigid node's PreviousObjectToWorld is the first pose's ObjectToWorld, bit for bit, its pixels carry
    motion and the static floor carries none. "None" is what CalculateMotionVector (GBufferGeneration.hlsl:62-91, restated bit for bit by
    k_gbuffer) can give a point that did not move: it re-projects the point and subtracts the pixel's own coordinate, so a static pixel keeps
    the rounding of that re-projection -- measured here: one fp32 rounding of a coordinate in [0, 1], 64 * 2^-24 = 3.8e-6 pixels. The bound
    below allows the eight roundings of the expression (clip / w, * 0.5 + 0.5, the subtraction, the scaling and the fp16 store); the box's
    motion must exceed it a thousandfold."""
    L = pkg.layouts
    a = Stage(ptamd, pkg)
    try:
        a.animation.SetTime(0.3)
        a.scene.Animate(a.animation)
        first = _instance_data(a, L)
        assert np.array_equal(first["PreviousObjectToWorld"].view(np.uint32), first["ObjectToWorld"].view(np.uint32))     # an object's first evaluation
        a.frame()
        a.animation.Tick(0.3)
        a.scene.Animate(a.animation)
        second = _instance_data(a, L)
        assert np.array_equal(second["PreviousObjectToWorld"][3].view(np.uint32), first["ObjectToWorld"][3].view(np.uint32))
        assert not np.array_equal(second["ObjectToWorld"][3], first["ObjectToWorld"][3])
        out = a.frame(frame_index=1)
        mv = out["MotionVector"].view(np.float16)[..., :2].astype(np.float32)
        base = out["BaseColorMetalness"]
        hit = np.isfinite(out["Position"][..., 0])
        box = hit & (base[..., 0] == 51) & (base[..., 2] == 204)          # the box's base colour (0.2, 0.5, 0.8)
        floor = hit & (base[..., 0] == 186) & (base[..., 1] == 186) & (base[..., 2] == 186)
        assert box.sum() >= 4 and floor.sum() >= 100, (int(box.sum()), int(floor.sum()))
        still = 8 * W * 2.0 ** -24                                        # pixels: the re-projection's rounding on a point that did not move
        print("motion on the static floor (max, pixels):", float(np.abs(mv[floor]).max()), "bound", still, "| on the box (min):", float(np.abs(mv[box]).max(-1).min()))
        assert np.all(np.abs(mv[box]).max(-1) > 1000 * still), "a pixel of the moving box carries no motion"
        assert np.all(np.abs(mv[floor]) <= still), "the static floor carries motion"
    finally:
        a.close()


def test_steady_state_allocates_nothing_and_every_frame_equals_a_fresh_context(ptamd, pkg):
    import torch
    a = Stage(ptamd, pkg)
    try:
        times, frames, stats = [], [], []
        for k in range(20):
            a.animation.Tick(0.07) if k else a.animation.SetTime(0.02)
            times.append(a.animation.times[0])
            a.scene.Animate(a.animation)
            frames.append(a.frame(frame_index=k))
            st = a.ctx.accel_stats()
            stats.append((st.NodeBytes, st.TriangleBytes, st.BlobBytes, st.OwnedBottomLevelBytes, torch.cuda.memory_allocated(0)))
        assert any(t1 < t0 for t0, t1 in zip(times, times[1:])), "the clock never wrapped through the clip's duration"
        assert len(set(stats[2:])) == 1, "device memory moved after frame 2"
        for k in range(20):                                              # the same two poses on a fresh context: the frame before it, then the frame
            f = Stage(ptamd, pkg)
            try:
                for t in times[max(0, k - 1):k + 1]:
                    f.animation.times[0] = t
                    f.scene.Animate(f.animation)
                _same_frame(frames[k], f.frame(frame_index=k), k)
            finally:
                f.close()
    finally:
        a.close()


def test_both_hosts_render_the_same_animated_frame(ptamd, pkg, tmp_path):
    """pt_demo --scene fixture --anim-time 0.37 writes the radiance bytes of ingest.load_scene + Scene.Animate at 0.37 s"""
    import dxpbrt_amd.ingest as I
    fixture = os.path.join(ROOT, "tests", "golden", "anim", "scene.json")
    demo = os.path.join(ROOT, "directx-physically-based-raytracer_amd", "pt_demo")
    out = str(tmp_path / "radiance.bin")
    subprocess.run([demo, "--scene", fixture, "--anim-time", "0.37", "--width", str(W), "--height", str(H), "--spp", "1", "--bounces", "3", "--frames", "1", "--out", out],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    a = Stage(ptamd, pkg, scene=I.load_scene(fixture, aspect=W / H))
    try:
        a.animation.SetTime(0.37)
        a.scene.Animate(a.animation)
        want = a.frame()["RadianceF32"]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        static = Stage(ptamd, pkg, scene=I.load_scene(fixture, aspect=W / H), animate=False)      # and the pose is what is being compared
        try:
            assert not np.array_equal(static.frame()["RadianceF32"], want)
        finally:
            static.close()
    finally:
        a.close()


# -------------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_rendered_frame_unchanged(ptamd, pkg):
    S = pkg.scenes
    a = Stage(ptamd, pkg)
    try:
        a.animation.SetTime(0.4)
        a.scene.Animate(a.animation)
        before = a.frame()
        ctx, lib = a.ctx, a.ctx.lib
        good = a.desc.animations[0]
        rig = good.rig

        def bad_rig(**changes):
            r = S.Rig(rig.parents.copy(), rig.rest.copy(), rig.durations.copy(), rig.channels.copy(), rig.key_times.copy(), rig.key_values.copy())
            for k, (index, value) in changes.items():
                getattr(r, k)[index] = value
            return [S.AnimatedObject(r, good.transform, good.binding_nodes, good.binding_instances, good.binding_globals, good.skins)]

        def bad_object(**changes):
            o = S.AnimatedObject(rig, good.transform, good.binding_nodes.copy(), good.binding_instances.copy(), good.binding_globals,
                                 [S.Skin(good.skins[0].mesh_node, good.skins[0].joint_nodes.copy(), good.skins[0].inverse_binds)])
            for k, (index, value) in changes.items():
                (o.skins[0].joint_nodes if k == "joint_nodes" else getattr(o, k))[index] = value
            return [o]

        first_key = int(rig.channels[0, 3, 1, 0])
        creations = {
            "Parent >= own index": bad_rig(parents=(2, 3)),
            "key times not strictly ascending": bad_rig(key_times=(first_key + 1, rig.key_times[first_key])),
            "key time not finite": bad_rig(key_times=(first_key + 2, np.inf)),
            "key value not finite": bad_rig(key_values=((first_key, 1), np.nan)),
            "rest TRS not finite": bad_rig(rest=((1, 4), np.inf)),
            "channel beyond the keys": bad_rig(channels=((1, 2, 1, 1), len(rig.key_times) + 1)),
            "node index out of range": bad_object(binding_nodes=(0, 5)),
            "joint index out of range": bad_object(joint_nodes=(1, 99)),
        }
        for what, objects in creations.items():
            with pytest.raises(ptamd.PtInvalidArgument):
                ptamd.Animation(ctx, objects)
            _same_frame(before, a.frame(), what)

        state = ptamd.AnimState(a.animation.handles[0], 0, 0, 0.4)
        inst = C.c_void_p(a.scene.instance_data.data_ptr())
        evaluate = lambda s, n=1: lib.pt_anim_evaluate(ctx.handle, C.addressof(s), n, inst)
        out = C.c_uint64(0)
        eye = np.eye(4, dtype=np.float32)
        far = ptamd.Animation(ctx, bad_object(binding_instances=(1, 1000)))                          # created; refused where the instance data is known
        twice = (ptamd.AnimState * 2)(state, state)
        calls = {
            "clip out of range": lambda: evaluate(ptamd.AnimState(a.animation.handles[0], 2, 0, 0.4)),
            "Time not finite": lambda: evaluate(ptamd.AnimState(a.animation.handles[0], 0, 0, float("nan"))),
            "unknown object id": lambda: evaluate(ptamd.AnimState(987654, 0, 0, 0.4)),
            "an object twice": lambda: lib.pt_anim_evaluate(ctx.handle, C.addressof(twice), 2, inst),
            "instance index out of range": lambda: evaluate(ptamd.AnimState(far.handles[0], 0, 0, 0.4)),
            "instance array not the bound one": lambda: lib.pt_anim_evaluate(ctx.handle, C.addressof(state), 1, C.c_void_p(a.scene.object_data.data_ptr())),
            "unknown rig id": lambda: lib.pt_anim_create_object(ctx.handle, 987654, C.c_void_p(eye.ctypes.data), 0, None, None, None, 0, None, None, None, None, C.byref(out)),
            "rig still referenced": lambda: lib.pt_anim_release_rig(ctx.handle, next(iter(a.animation.rigs.values()))),
            "unknown rig released": lambda: lib.pt_anim_release_rig(ctx.handle, 987654),
            "unknown object released": lambda: lib.pt_anim_release_object(ctx.handle, 987654),
            "posed top level without instance data": lambda: lib.pt_build_top_level_posed(ctx.handle, C.addressof(a.scene._descs), len(a.desc.objects), 0x4, None,
                                                                                          C.c_void_p(a.animation.from_device(len(a.desc.objects)).ctypes.data)),
        }
        for what, call in calls.items():
            assert call() == -1, what                                     # PT_ERROR_INVALID_ARGUMENT
            assert lib.pt_last_error(ctx.handle), what
            _same_frame(before, a.frame(), what)
        far.close()
        a.scene.Animate(a.animation)                                      # and the good call still works, to the same image (the motion is now nil)
        after = a.frame()
        for k in ("Position", "RadianceF32", "rays"):
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    finally:
        a.close()
