"""CPU tests: the C-ABI library loads without a GPU, exports every symbol include/ptamd.h declares, fails
loudly without a device, and the host-side layouts / scene flattening / sharding logic are right."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pt_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(ptamd):
    lib = ptamd.load_library()
    names = declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"libptamd.so does not export {n}"
    assert sorted(ptamd.EXPORTS) == names                       # the Python binding covers the whole header
    assert lib.pt_abi_version() == 4


def test_struct_sizes_match_reference_layouts(pkg, ptamd):
    L = pkg.layouts
    assert L.VERTEX.itemsize == 32 and L.OBJECT_DATA.itemsize == 224 and L.INSTANCE_DATA.itemsize == 112
    assert L.SCENE_DATA.itemsize == 80 and L.CAMERA.itemsize == 608 and L.MATERIAL.itemsize == 64
    assert L.GRAPHICS_SETTINGS.itemsize == 80 and L.GBUFFER_CONSTANTS.itemsize == 12
    assert L.OBJECT_DATA.fields["Material"][1] == 48 and L.OBJECT_DATA.fields["TextureMapInfoArray"][1] == 112
    assert L.CAMERA.fields["WorldToProjection"][1] == 416 and L.CAMERA.fields["Jitter"][1] == 88
    assert L.INSTANCE_DATA.fields["ObjectToWorld"][1] == 64
    assert C.sizeof(ptamd.GeometryDesc) == 40 and C.sizeof(ptamd.InstanceDesc) == 64
    assert C.sizeof(ptamd.Textures) == 17 * 8 and C.sizeof(ptamd.Counters) == 64
    # the BSDF building blocks: flat float arrays of 20 / 8 / 24 / 12 words in the tests and the oracle
    assert C.sizeof(ptamd.BsdfQuery) == 80 and C.sizeof(ptamd.BsdfResult) == 32
    assert C.sizeof(ptamd.BsdfSampleQuery) == 96 and C.sizeof(ptamd.BsdfSampleResult) == 48
    for s, name, off in ((ptamd.BsdfQuery, "GeometricNormal", 32), (ptamd.BsdfQuery, "L", 68),
                         (ptamd.BsdfResult, "PDF", 24), (ptamd.BsdfSampleQuery, "GeometricNormal", 32),(ptamd.BsdfSampleQuery, "V", 56),
                         (ptamd.BsdfSampleQuery, "Random", 68), (ptamd.BsdfSampleQuery, "ExtFlags", 84),
                         (ptamd.BsdfSampleResult, "F", 16), (ptamd.BsdfSampleResult, "Weights", 28),
                         (ptamd.BsdfSampleResult, "Lobe", 40), (ptamd.BsdfSampleResult, "Ok", 44)):
        assert getattr(s, name).offset == off, (s.__name__, name)


def test_fails_loudly_without_gpu(ptamd):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(ptamd.PtError) as e:
        ptamd.DeviceContext(0)
    assert "no HIP device" in str(e.value) or "no CPU fallback" in str(e.value)


def test_product_does_not_touch_the_oracle():
    """the product path must not import / link / include anything under oracle/."""
    pkg_dir = os.path.join(ROOT, "directx-physically-based-raytracer_amd")
    for base, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp", "Makefile")):
                text = open(os.path.join(base, f), errors="ignore").read()
                assert "pt_oracle" not in text and "load_oracle" not in text and "oracle/" not in text, os.path.join(base, f)
    text = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    assert "oracle" not in text.lower()


def test_scene_flattening(pkg):
    S, L = pkg.scenes, pkg.layouts
    sc = S.cornell_box(glass_sphere=True)
    assert len(sc.objects) == 9 and len(sc.object_data) == 9 and sc.triangle_count == 2 * 6 + 12 * 2 + 320
    # InstanceID = FirstGeometryIndex, one ObjectData per (instance, geometry) (Scene.ixx:216-228, App.cpp:1028-1074)
    assert list(sc.instance_ids) == list(range(9))
    assert np.all(sc.object_data["VertexDesc"]["Stride"] == 32) and np.all(sc.object_data["VertexDesc"]["Normal"] == 12)
    assert np.all(sc.object_data["TextureMapInfoArray"]["Descriptor"] == L.NONE)
    light = sc.object_data[5]["Material"]
    assert light["EmissiveStrength"] == 15 and tuple(light["EmissiveColor"]) == (1, 1, 1)
    multi = S.sponza_scale(n_side=24)
    assert multi.blas[0][1] == len(multi.nodes[0].meshes) > 1   # many geometries in one BLAS
    assert list(multi.instance_ids) == [0, multi.blas[0][1]]
    # u16 / u32 index choice (GLTFHelpers.ixx:183-188)
    assert S.make_indices(np.zeros(65535)).dtype == np.uint16 and S.make_indices(np.zeros(65538)).dtype == np.uint32
    nn = S.cornell_box(has_normals=False)
    assert np.all(nn.object_data["VertexDesc"]["Normal"] == L.NONE)


def test_camera_matches_controller_semantics(pkg):
    S = pkg.scenes
    cam = S.make_camera((1, 2, 3), forward=(0, 0, 1), hfov_deg=90.0, aspect=2.0, near=0.01)
    assert np.allclose(cam["RightDirection"], (1, 0, 0)) and np.allclose(cam["UpDirection"], (0, 0.5, 0))   # |Right| = tan(hfov/2), |Up| = |Right|/aspect
    p = np.array([1.5, 2.25, 7.0, 1.0])
    clip = p @ cam["WorldToProjection"].astype(np.float64)
    assert np.isclose(clip[3], 4.0) and np.isclose(clip[2], 0.01)     # w = view depth, reversed-Z infinite: z = near
    assert np.allclose(clip[:2] / clip[3], (0.125, 0.125))
    assert np.allclose(cam["WorldToProjection"].astype(np.float64) @ np.linalg.inv(cam["WorldToProjection"].astype(np.float64)), np.eye(4), atol=1e-5)


def test_sharding_helpers_match_library(ptamd):
    ge_pkg = __import__("dxpbrt_amd.sharding", fromlist=["x"])
    for H in (1080, 2160, 37, 16, 5):
        for world in (1, 2, 3, 4, 8):
            for band in (1, 8, 16):
                rows = [ge_pkg.local_rows(H, r, world, band) for r in range(world)]
                assert sum(rows) == H
                assert rows == [ptamd.local_rows(H, r, world, band) for r in range(world)]
    full = np.arange(37 * 3).reshape(37, 3)
    pieces = [ge_pkg.extract_local(full, r, 4, 8) for r in range(4)]
    assert np.array_equal(ge_pkg.deinterleave(pieces, 37, 8), full)
    with pytest.raises(ptamd.PtInvalidArgument):
        ptamd.local_rows(10, 3, 2, 16)


def test_gather_plans_pair_up_and_tile_the_frame(ptamd):
    """pt_gather_plan (the host arithmetic of pt_gather_bands, no GPU): over all ranks, every ncclSend meets an ncclRecv of the
    same size in the same order per peer, the receives plus the root's own bands cover every row of the frame exactly once, and
    the local offsets walk each sender's texture contiguously."""
    ge_pkg = __import__("dxpbrt_amd.sharding", fromlist=["x"])
    for H, W, px in ((1080, 1920, 8), (2160, 3840, 8), (37, 6, 16), (16, 2, 8), (5, 4, 8)):
        row = W * px
        for world in (1, 2, 3, 8):
            for band in (4, 16):
                for root in sorted({0, world - 1}):
                    plans = [ptamd.gather_plan(H, row, r, world, band, root) for r in range(world)]
                    recvs = plans[root]
                    assert all(not m[1] for m in recvs)
                    covered = np.zeros(H, np.int32)
                    for y0, y1, _ in ge_pkg.rank_bands(H, root, world, band):
                        covered[y0:y1] += 1                                   # the root's own bands never travel
                    for r in range(world):
                        if r == root:
                            continue
                        sends = plans[r]
                        assert all(m[1] == 1 and m[0] == root for m in sends)
                        mine = [m for m in recvs if m[0] == r]
                        assert [(m[2], m[5], m[4]) for m in mine] == [(m[2], m[5], m[4]) for m in sends]     # same bands, sizes, destinations, same order
                        off = 0
                        for (_, _, b, lo, fo, n), (y0, y1, l0) in zip(sends, ge_pkg.rank_bands(H, r, world, band)):
                            assert lo == off == l0 * row and fo == y0 * row and n == (y1 - y0) * row and b == y0 // band
                            off += n
                            covered[y0:y1] += 1
                        assert off == ge_pkg.local_rows(H, r, world, band) * row
                    assert np.all(covered == 1)
    with pytest.raises(ptamd.PtInvalidArgument):
        ptamd.gather_plan(16, 64, 0, 2, 16, root=2)


def test_textured_sponza_scale_scene(pkg, oracle):
    """scenes.sponza_scale(textured=True), the workload of `bench.py --workload c3t` (BASELINE configs[2] says "Sponza-scale glTF"): the geometry of
    the untextured scene, plus UVs, tangents, three textures per material and three alpha-masked strips -- checked here at a small size on
    the CPU (the full size runs under -m gpu): layout of the heap and the object data, and that the oracle sees through the lattice."""
    S, L = pkg.scenes, pkg.layouts
    plain = S.sponza_scale(n_side=48, aspect=2.0)
    tex = S.sponza_scale(n_side=48, aspect=2.0, textured=True, texture_size=32)
    assert tex.triangle_count == plain.triangle_count
    assert np.array_equal(tex.nodes[0].meshes[7].vertices["Position"], plain.nodes[0].meshes[7].vertices["Position"])
    kinds = [h.kind for h in tex.heap]
    assert kinds.count(S.KIND_TEXTURE2D) == 3 * 24 and kinds.count(S.KIND_BUFFER) == 2 * 25
    od = tex.object_data
    assert int((od["Material"]["AlphaMode"] == 1).sum()) == 3
    used = od["TextureMapInfoArray"]["Descriptor"][:24] != L.NONE
    assert used[:, [0, 4, 6]].all() and not used[:, [1, 2, 3, 5]].any()             # BaseColor, MetallicRoughness, Normal
    assert np.all(od["VertexDesc"]["Tangent"][:24] == 18) and np.all(od["VertexDesc"]["TexCoord"][:24, 0] == 24)
    W, H = 96, 48
    gs = S.graphics_settings(W, H, spp=1, bounces=2)
    tex.scene_data = S.make_scene_data((0.2, 0.3, 0.4, 1.0))
    a, rays_a, _ = oracle.render(tex, gs, accel_mode=1, layouts=L)
    for m in tex.nodes[0].meshes:
        m.material["AlphaMode"] = 0
    tex.finalize()
    b, rays_b, _ = oracle.render(tex, gs, accel_mode=1, layouts=L)
    assert rays_a > 0 and not np.array_equal(a["Position"], b["Position"])          # some primary rays pass through the masked strips' cut-outs
