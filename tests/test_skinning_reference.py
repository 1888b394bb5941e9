"""k_skin (csrc/pt_skin.hip) and the oracle's or_skin_mesh against the float64 restatement of the skinning rule in tests/skinref.py.

The existing tests compare the kernel with or_skin_mesh only -- the same fp32 arithmetic written twice -- on a mesh with two joints,
a zero implied weight and rigid poses, where the normal rule and the tangent rule coincide. Here the inputs have four distinct joints
per vertex, Dirichlet weights, a negative implied weight, non-uniform scale and mirrored joints, and the bounds are derived in
skinref's docstring, not measured. `test_every_mutation_breaks_a_bound` is the self-test: each wrong rule in skinref.MUTATIONS must
break a bound on these very inputs.

Figures observed (the bounds are skinref.POSITION_ULPS = 16, LSB_BOUND = 1, LSB_SHARE_BOUND = 2 %, 0.5 ulp_fp16, COND_CAP = 2000):
  or_skin_mesh, CPU, 330 vertices, 6 joints:  position error <= 1.95 * 2^-24 S; normals / tangents differ by <= 1 LSB in 0.30 % of the
                                              components; motion <= 0.497 ulp_fp16 over the position bound; cond(M3x3) <= 5.9
  k_skin, MI355X, 1000 vertices, 6 joints:    position error <= 1.66 * 2^-24 S; normals / tangents differ by <= 1 LSB in 0.13 % of the
                                              components; motion <= 0.498 ulp_fp16 over the position bound; cond(M3x3) <= 6.3
The kernel's bytes equal or_skin_mesh's at every count and pose kind.
"""
import ctypes as C

import numpy as np
import pytest

import skinref

JOINTS = 6
FIRST = ("rigid", 101)              # the pose skinned first: motion then reads a non-rest previous position of order one
SEED = 7
CHECKED_KINDS = [k for k in skinref.KINDS if k != "flat"]


def oracle_skin(oracle, mesh, transforms):
    tr = np.ascontiguousarray(transforms, np.float32)
    oracle.lib().or_skin_mesh(mesh.skeletal_vertices.ctypes.data, tr.ctypes.data, mesh.vertices.ctypes.data,
                              mesh.motion_vectors.ctypes.data, len(mesh.vertices))


def oracle_run(oracle, n_triangles, kind):
    """rest -> FIRST -> kind by the oracle. Returns (mesh, positions before the last pose, transforms of the last pose)."""
    mesh = skinref.skinned_strip(n_triangles, JOINTS, SEED)
    oracle_skin(oracle, mesh, skinref.poses(JOINTS, *FIRST))
    prev = mesh.vertices["Position"].copy()
    tr = skinref.poses(JOINTS, kind, SEED)
    oracle_skin(oracle, mesh, tr)
    return mesh, prev, tr


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    return {kind: oracle_run(oracle, 328, kind) for kind in CHECKED_KINDS}


def test_inputs_tell_the_rules_apart():
    mesh = skinref.skinned_strip(328, JOINTS, SEED)
    sk = mesh.skeletal_vertices
    assert mesh.indices.size == 3 * 328 and int(mesh.indices.max()) == len(sk) - 1
    assert skinref.skinned_strip(33, JOINTS, SEED).indices.size == 99          # an odd count drops the last triangle
    assert all(len(set(j.tolist())) == 4 for j in sk["Joints"])
    w3 = 1.0 - sk["Weights"][:, :3].astype(np.float64).sum(1)
    assert w3[1] == 0.0 and w3[2] == 1.0 and w3[3] == -0.5
    assert (np.abs(w3 - sk["Weights"][:, 3]) > 1e-3).mean() > 0.9                # the stored fourth weight is not the implied one
    for kind in ("scale", "mirror"):
        A = skinref.poses(JOINTS, kind, SEED)[:, :, :3].astype(np.float64)
        assert all(np.abs(np.linalg.inv(a).T - a).max() > 1e-2 for a in A) or kind == "mirror"
        if kind == "mirror":
            assert (np.linalg.det(A) < 0).all()


def test_oracle_skinning_within_the_float64_bounds(oracle_runs):
    worst = {}
    for kind, (mesh, prev, tr) in oracle_runs.items():
        ref = skinref.skin_reference(mesh.skeletal_vertices, tr, prev)
        normals = kind in skinref.NORMAL_KINDS
        if normals:
            assert ref["cond"].max() <= skinref.COND_CAP
        m = skinref.measure(ref, mesh.vertices, mesh.motion_vectors, normals)
        print(f"or_skin_mesh {kind}: {m}")
        assert not skinref.violations(m), (kind, skinref.violations(m))
        for k, v in m.items():
            if v is not None:
                worst[k] = max(worst.get(k, v), v)
    print(f"or_skin_mesh worst: {worst}")


@pytest.mark.parametrize("mutation", skinref.MUTATIONS)
def test_every_mutation_breaks_a_bound(oracle_runs, mutation):
    """The bounds' self-test: against a reference that follows a wrong rule, the (right) oracle output must break a bound."""
    broken = []
    for kind, (mesh, prev, tr) in oracle_runs.items():
        ref = skinref.skin_reference(mesh.skeletal_vertices, tr, prev, mutation=mutation)
        m = skinref.measure(ref, mesh.vertices, mesh.motion_vectors, kind in skinref.NORMAL_KINDS)
        if skinref.violations(m):
            broken.append(kind)
    assert broken, f"the inputs are too weak to notice '{mutation}'"


def test_motion_vector_is_old_minus_new_in_half(oracle_runs):
    for kind, (mesh, prev, tr) in oracle_runs.items():
        mv32 = prev - mesh.vertices["Position"]
        assert np.array_equal(mesh.motion_vectors[:, :3], mv32.astype(np.float16).view(np.uint16)), kind


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------
GPU_TRIANGLES = 998                  # 1000 vertices
MOTION_FILL = 0x3C5A                 # what the motion buffer holds before: .w and the vertices beyond `count` must keep it


@pytest.fixture(scope="module")
def gpu_oracle_runs(oracle):
    return {kind: oracle_run(oracle, GPU_TRIANGLES, kind) for kind in CHECKED_KINDS}


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000])
def test_gpu_skinning_against_float64(gpu, ptamd, gpu_oracle_runs, count):
    """pt_skin_mesh on the first `count` vertices (the lone vertex, the grid's tail on either side of a block, several blocks): within
    the float64 bounds, byte-equal to or_skin_mesh, motion = half(previous - new) of the downloaded positions, and nothing else
    written: texture coordinates, motion.w and every vertex beyond `count` keep their bytes."""
    import torch
    rest = skinref.skinned_strip(GPU_TRIANGLES, JOINTS, SEED)
    assert len(rest.vertices) == 1000
    dev = torch.device("cuda", gpu.device_ordinal)
    sk = ptamd.to_device(rest.skeletal_vertices, dev)
    rest_motion = np.full((len(rest.vertices), 4), MOTION_FILL, np.uint16)
    worst = {}
    for kind in CHECKED_KINDS:
        host, host_prev, tr = gpu_oracle_runs[kind]
        dv = ptamd.to_device(rest.vertices, dev)
        dm = ptamd.to_device(rest_motion, dev)
        downloads = []
        for pose in (skinref.poses(JOINTS, *FIRST), tr):
            dt = ptamd.to_device(pose, dev)
            gpu.check(gpu.lib.pt_skin_mesh(gpu.handle, C.c_void_p(sk.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_void_p(dv.data_ptr()),
                                           C.c_void_p(dm.data_ptr()), count))
            gpu.sync()
            downloads.append((dv.cpu().numpy().view(rest.vertices.dtype).copy(), dm.cpu().numpy().view(np.uint16).reshape(-1, 4).copy()))
        (v1, _), (v2, m2) = downloads
        prev = v1["Position"][:count]
        ref = skinref.skin_reference(rest.skeletal_vertices[:count], tr, prev)
        normals = kind in skinref.NORMAL_KINDS
        if normals:
            assert ref["cond"].max() <= skinref.COND_CAP
        m = skinref.measure(ref, v2[:count], m2[:count], normals)
        print(f"k_skin count={count} {kind}: {m}")
        assert not skinref.violations(m), (kind, skinref.violations(m))
        for k, v in m.items():
            if v is not None:
                worst[k] = max(worst.get(k, v), v)
        # motion from two downloads, bit for bit
        assert np.array_equal(m2[:count, :3], (prev - v2["Position"][:count]).astype(np.float16).view(np.uint16)), kind
        # nothing else written
        raw2, raw0 = v2.view(np.uint8).reshape(-1, 32), rest.vertices.view(np.uint8).reshape(-1, 32)
        assert np.array_equal(raw2[:, 24:], raw0[:, 24:]), kind
        assert np.array_equal(raw2[count:], raw0[count:]), kind
        assert (m2[:, 3] == MOTION_FILL).all() and (m2[count:] == MOTION_FILL).all(), kind
        # and the same bytes as the oracle (which skinned all 1000 vertices through the same two poses)
        assert np.array_equal(prev, host_prev[:count]), kind
        assert np.array_equal(raw2[:count], host.vertices.view(np.uint8).reshape(-1, 32)[:count]), kind
        assert np.array_equal(m2[:count, :3], host.motion_vectors[:count, :3]), kind
    print(f"k_skin count={count} worst: {worst}")
