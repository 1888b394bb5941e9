"""GPU tests of the SHARC radiance cache (pt_sharc_*, pt_raytrace_render_sharc) against the numpy restatement of its rules
(tests/sharcref.py) and against the unchanged plain path tracer.

What is exact: keys, the {key -> voxel} map after every update + resolve, the query decision (cases within sharcref.NEAR of a decision are
left out and counted, at most 1 %), an empty cache against the plain render (bit for bit, ray counters included), determinism.
What is bounded: an empty cache with DI on (the DI term enters the sum per sample instead of once after the division: see
test_di_on), and the end-to-end image (the cache is biased by voxel averaging, the roughness floor and the 1e-3 quantisation, so the
tolerance is measured, not derived: see test_end_to_end)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import dipins
import sharcref as R

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
LOG_PATHS, SKIP_UPDATE, UNFUSED = 0x100, 0x200, 0x10
M32 = 0xFFFFFFFF

# test_end_to_end, measured on one MI355X (diffuse Cornell 192 x 108, 8 bounces, 64 frames from an empty cache; differences of 4 x 4 region
# means and of the whole-image mean, relative to the yardstick's whole-image mean):
#   the plain tracer against itself on two disjoint FrameIndex sets (16 spp x 64 frames each)   regions 0.0109   whole image 0.0017
#   the cache (1 spp x 64 frames, reference defaults) against the yardstick                     regions 0.0225   whole image 0.0015
E2E_SPREAD_REGION, E2E_SPREAD_IMAGE = 0.0109, 0.0017
E2E_OFFSET_REGION, E2E_OFFSET_IMAGE = 0.0225, 0.0015


def _hash(x):
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32; x ^= x >> 15; x = (x * 0x846CA68B) & M32; x ^= x >> 16
    return x


def rng_init(px, py, frame):
    seed = _hash((frame + 0x035F9F29) & M32)
    v = ((px << 16) | (py & 0xFFFF)) & M32
    return seed ^ ((_hash(v) + 0x9E3779B9 + (seed << 6) + (seed >> 2)) & M32)


def rng_float(st):
    st = (st * 1664525 + 1013904223) & M32
    return st, np.float32(_hash(st) >> 8) * np.float32(1.0 / 16777216.0)


class Rig:
    """a context of its own (debug flags and the cache do not leak into other tests), a scene and a renderer"""

    def __init__(self, ptamd, scene, W, H, capacity=1 << 16, flags=0, denoiser_outputs=False, shared_from=None):
        self.ptamd, self.W, self.H = ptamd, W, H
        self.ctx = ptamd.DeviceContext(0)
        self.ctx.set_debug_flags(flags)
        self.scene = ptamd.SharedScene(self.ctx, shared_from.scene) if shared_from is not None else ptamd.Scene(self.ctx, scene)
        self.r = ptamd.Renderer(self.ctx, self.scene, W, H, with_f32=True, with_denoiser_outputs=denoiser_outputs)
        if capacity is not None:
            self.r.sharc.Configure(capacity)

    def frame(self, gs, sharc=None, **kw):
        self.ctx.reset_counters()
        self.r.render(gs, sharc=sharc, **kw)
        self.ctx.sync()
        t = self.ptamd.textures_to_numpy({k: self.r.textures[k] for k in ("Radiance", "RadianceF32")})
        c = self.ctx.counters()
        return t["Radiance"].copy(), t["RadianceF32"].copy(), (c.PrimaryRays, c.SecondaryRays)

    def map(self):
        e = self.r.sharc.download()
        return {int(k): [int(x) for x in v] for k, v in zip(e["Key"], e["Voxel"])}

    def close(self):
        self.ctx.close()


@pytest.fixture
def rigs():
    made = []
    yield made
    for r in made:
        r.close()


def settings(pkg, W, H, spp=1, bounces=8, frame=0, **kw):
    gs = pkg.scenes.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=frame)
    for k, v in kw.items():
        gs[k] = v
    return gs


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------
def test_keys(ptamd, pkg):
    L = pkg.layouts
    ctx = ptamd.DeviceContext(0)
    try:
        sh = ptamd.SHARC(ctx)
        rng = np.random.default_rng(20240607)
        left_out = total = 0
        for cam_pos, scale in (((0.0, 0.0, -1.95), 50.0), ((3.0, -2.0, 5.0), 50.0), ((-40.0, 10.0, 25.0), 17.5), ((0.25, 0.5, -0.125), 100.0)):
            cam = pkg.scenes.make_camera(cam_pos)
            ctx.check(ctx.lib.pt_set_camera(ctx.handle, C.c_void_p(np.array(cam).ctypes.data)))
            sh.SetConstants(L.sharc_settings(scene_scale=scale))
            n = 50000
            d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
            lo = max(0.05, np.linalg.norm(cam_pos) / 4)
            dist = np.exp(rng.uniform(np.log(lo), np.log(2000.0), n))
            pos = (np.asarray(cam_pos)[None, :] + d * dist[:, None]).astype(np.float32)
            nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
            nrm[::7] = np.eye(3)[rng.integers(0, 3, len(nrm[::7]))] * rng.choice([-1.0, 1.0], len(nrm[::7]))[:, None]   # axis-aligned walls
            nrm = nrm.astype(np.float32)
            keys, levels, sizes, near = R.grid(np.array(cam)["Position"], pos, nrm, scale)
            gk, gl, gs_ = sh.debug_keys(pos, nrm)
            ok = ~near
            assert np.array_equal(gk[ok], keys[ok]) and np.array_equal(gl[ok], levels[ok]) and np.array_equal(gs_[ok], sizes[ok])
            assert len(set(levels.tolist())) >= 8                       # several levels are in play
            left_out += int(near.sum()); total += n
        print(f"keys: {left_out} of {total} left out near a decision ({left_out / total:.4%})")
        assert left_out <= 0.01 * total
    finally:
        ctx.close()


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_ggx", "cornell_textured", "instanced_grid"])
@pytest.mark.parametrize("flags", [0, UNFUSED])
def test_empty_cache_is_the_plain_render(ptamd, pkg, rigs, name, flags):
    S = pkg.scenes
    W, H = 256, 144
    scene = {"cornell_ggx": lambda: S.cornell_box(aspect=W / H, variant="ggx", glass_sphere=True),
             "cornell_textured": lambda: S.cornell_box_textured(aspect=W / H),
             "instanced_grid": lambda: S.instanced_grid(n=12, aspect=W / H, subdiv=1)}[name]()
    rig = Rig(ptamd, scene, W, H, flags=flags | SKIP_UPDATE); rigs.append(rig)
    gs = settings(pkg, W, H, spp=2, bounces=5, frame=3)
    plain = rig.frame(gs)
    cached = rig.frame(gs, sharc=pkg.layouts.sharc_settings())
    assert plain[2][1] > 0
    assert np.array_equal(plain[0], cached[0]) and np.array_equal(plain[1].view(np.uint32), cached[1].view(np.uint32))
    assert plain[2] == cached[2]
    assert len(rig.map()) == 0


def test_no_update_pixel_leaves_the_plain_render(ptamd, pkg, rigs):
    """5 x 3 with DownscaleFactor 4: the update grid is 1 x 0, so no update pass runs (the resolve and the query do, on an empty map).
    The map stays empty and the frame is the plain render bit for bit, ray counters included -- with no debug flag to keep the cache empty."""
    S = pkg.scenes
    W, H = 5, 3
    rig = Rig(ptamd, S.cornell_box(aspect=W / H, variant="ggx", glass_sphere=True), W, H); rigs.append(rig)
    for f in range(2):
        gs = settings(pkg, W, H, spp=8, bounces=5, frame=3 + f)
        plain = rig.frame(gs)
        cached = rig.frame(gs, sharc=pkg.layouts.sharc_settings(downscale=4))
        assert plain[2] == (W * H, plain[2][1]) and plain[2][1] > 0
        assert np.array_equal(plain[0], cached[0]) and np.array_equal(plain[1].view(np.uint32), cached[1].view(np.uint32))
        assert plain[2] == cached[2]
        assert len(rig.map()) == 0 and rig.r.sharc.download_update_paths().size == 0


# ---- 3, 4, 5 -----------------------------------------------------------------------------------------------------------------------
# The update pass runs one path per update pixel, (W / DownscaleFactor) x (H / DownscaleFactor) of them, truncated. 64 x 36 halves evenly; 37 x 23 gives
# 18 x 11 (factor 2) and 12 x 7 (factor 3): both axes truncated, both grids cut the 16 x 16 block and the 8 x 8 wave tile, and the G-buffer texel of a
# path is min(int(u * W), W - 1) with an odd W.
# At 37 x 23 the camera is jittered by a fraction of a pixel (test_estimator_reference.py's jitter): unjittered, pixel centres of this raster lie on
# the seams between the walls, where a path starts inside the next wall's plane, meets it at t = 0 and can stay in the corner for several bounces --
# six of the 574 segments of the first frame, all too short for test_log_validity's probe, which allows 1 %.
PINNED = [((64, 36), 2), ((37, 23), 2), ((37, 23), 3)]
RAGGED_PINNED = PINNED[1:]
RAGGED_JITTER = (0.2, -0.35)
_pinned_id = lambda p: f"{p[0][0]}x{p[0][1]}-downscale{p[1]}"


def _pinned_frames(ptamd, pkg, rigs, frames=3, size=(64, 36), downscale=2):
    S, L = pkg.scenes, pkg.layouts
    W, H = size
    scene = S.cornell_box(aspect=W / H, variant="diffuse", jitter=(0.0, 0.0) if size == (64, 36) else RAGGED_JITTER)
    rig = Rig(ptamd, scene, W, H, capacity=1 << 16, flags=LOG_PATHS); rigs.append(rig)
    ss = L.sharc_settings(downscale=downscale, accumulation_frames=2)  # frame 2 is the third: the resolve's rescale is in the comparison
    ref = R.Cache(1 << 16)
    cam = np.array(scene.camera)["Position"]
    out = []
    for f in range(frames):
        rig.frame(settings(pkg, W, H, frame=f), sharc=ss)
        log = rig.r.sharc.download_update_paths()
        assert log.shape == ((W // downscale) * (H // downscale), 9)
        resampled = wrong_keys = vertices = 0
        for path in log:
            hit = (path["Flags"] & R.HIT) != 0
            logged = path["KeyLo"].astype(np.uint64) | (path["KeyHi"].astype(np.uint64) << np.uint64(32))
            keys, _, _, near = R.grid(cam, path["Position"], path["Normal"], float(ss["SceneScale"]))
            differ = hit & (keys != logged)
            assert not (differ & ~near).any()                           # the device's key is the restatement's, except within NEAR of a decision
            wrong_keys += int(differ.sum()); vertices += int(hit.sum())
            resampled += ref.update_path(path, np.where(differ, logged, keys))
            assert resampled >= 0
        assert ref.refused == 0 and ref.fullest_bucket() < R.BUCKET     # no bucket filled up: no vertex was dropped (drops depend on arrival order)
        ref.resolve(int(ss["AccumulationFrames"]), int(ss["MaxStaleFrames"]), bool(ss["IsAntiFireflyEnabled"]))
        got = rig.map()
        device_resampled = int(((log["Flags"] & R.RESAMPLED) != 0).sum())
        print(f"frame {f}: {vertices} vertices, {len(got)} live entries, {resampled} resampled terminations, {wrong_keys} keys within NEAR of a decision")
        assert device_resampled == resampled
        assert wrong_keys <= 0.01 * vertices
        assert got == ref.resolved                                      # integers, exactly
        out.append((log, resampled))
    return rig, ref, scene, ss, out


def test_update_and_resolve_pinned(ptamd, pkg, rigs):
    rig, ref, scene, ss, out = _pinned_frames(ptamd, pkg, rigs)
    assert len(ref.resolved) > 500
    assert out[2][1] >= 1                                               # frame 2 took the history at least once, or this proves nothing
    assert any(R.unpack(v[3])[1] == 2 and R.unpack(v[3])[2] == 0 for v in ref.resolved.values())   # ... and voxels went through the AccumulationFrames rescale


@pytest.mark.parametrize("pinned", RAGGED_PINNED, ids=_pinned_id)
def test_update_and_resolve_pinned_ragged(ptamd, pkg, rigs, pinned):
    """the same three frames where the update grid is truncated on both axes and cut by its blocks: keys, the resampled count and the
    {key -> voxel} map exact, as _pinned_frames asserts frame by frame (the floor on live entries is 64 x 36's share of the paths)"""
    (W, H), downscale = pinned
    rig, ref, scene, ss, out = _pinned_frames(ptamd, pkg, rigs, size=(W, H), downscale=downscale)
    assert dipins.more_than(len(ref.resolved), 500, W // downscale, H // downscale, 32, 18)
    assert out[2][1] >= 1
    assert any(R.unpack(v[3])[1] == 2 and R.unpack(v[3])[2] == 0 for v in ref.resolved.values())


def _log_validity(ptamd, pkg, rigs, pinned):
    """Vertex 0 is the G-buffer texel under the LOAD rule; the first two draws are the jitter and the hit update's random number;
    pt_bsdf_sample with the logged inputs (Roughness after the RoughnessThreshold floor) reproduces the next direction and, up to bounce 3
    (before Russian roulette), the throughput handed to SetThroughput; and every vertex sees the next one along the logged ray.
    The floors on segments and throughputs (500 at 64 x 36 / 2) are taken as the same share of the paths at the other sizes."""
    import torch
    (W, H), f = pinned
    rig, ref, scene, ss, out = _pinned_frames(ptamd, pkg, rigs, frames=1, size=(W, H), downscale=f)
    log = out[0][0]
    scatter = rig.r.sharc.download_update_scatter()
    assert scatter.shape == log.shape
    uw, uh = W // f, H // f
    more = lambda value, count: dipins.more_than(value, count, uw, uh, 32, 18)
    position = ptamd.textures_to_numpy({"Position": rig.r.textures["Position"]})["Position"]
    rays, steps, too_close, short = [], [], 0, []
    PROBE_CLEARANCE = 1e-4                                                # the probe ends this far above the next vertex's face
    for path_index, path in enumerate(log):
        ux, uy = path_index % uw, path_index // uw
        st, r0 = rng_float(rng_init(ux, uy, 0))                          # the first draw is the jitter
        j = np.float32(r0 - np.float32(0.5))
        u = np.float32(np.float32(np.float32(ux) + np.float32(0.5)) + j) / np.float32(uw)
        v = np.float32(np.float32(np.float32(uy) + np.float32(0.5)) + j) / np.float32(uh)
        px, py = min(int(np.float32(u * np.float32(W))), W - 1), min(int(np.float32(v * np.float32(H))), H - 1)
        texel = position[py, px]
        if not np.isfinite(texel[3]):
            assert int(path["Flags"][0]) == R.MISS | R.ENDED
            continue
        assert int(path["Flags"][0]) & R.HIT and np.array_equal(path["Position"][0].view(np.uint32), texel[:3].view(np.uint32))
        st, r1 = rng_float(st)
        assert path["Random"][0] == r1                                   # ... and the second the hit update's random number
        draws = []
        for _ in range(4):                                               # ... then the GetFloat4 of the BSDF sample
            st, r = rng_float(st); draws.append(r)
        if int(scatter[path_index, 0]["Sampled"]):
            assert np.array_equal(scatter[path_index, 0]["Query"].view(np.float32)[17:21], np.asarray(draws, np.float32))
        for b in range(len(path)):
            e = scatter[path_index, b]
            hit, ended = int(path["Flags"][b]) & R.HIT, int(path["Flags"][b]) & R.ENDED
            assert int(e["Sampled"]) == (1 if hit and not (int(path["Flags"][b]) & R.RESAMPLED) else 0)
            if not int(e["Sampled"]):
                continue
            assert int(e["Goes"]) == (0 if ended else 1)
            steps.append((path_index, b))
            if b + 1 < len(path) and int(path["Flags"][b + 1]) & R.HIT:
                o, d = e["Origin"].astype(np.float64), e["L"].astype(np.float64)
                nn = path["Normal"][b + 1].astype(np.float64)
                cos = abs(d @ nn)
                t_plane = ((path["Position"][b + 1].astype(np.float64) - o) @ nn) / (d @ nn)      # where the ray meets the next vertex's face
                tmax = t_plane - PROBE_CLEARANCE / cos
                if tmax <= 0:
                    too_close += 1
                    short.append((path_index, b, float(t_plane), float(cos)))
                    continue
                rays.append(np.concatenate([o, [0.0], d, [tmax]]))
    assert more(len(rays), 500) and len(steps) > len(rays)
    dev = torch.device("cuda", rig.ctx.device_ordinal)
    ctx, lib = rig.ctx, rig.ctx.lib
    # the BSDF step again, through pt_bsdf_sample
    q = np.ascontiguousarray(np.stack([scatter[p, b]["Query"] for p, b in steps]))
    rough = q.view(np.float32).reshape(len(steps), 24)[:, 4]
    assert (rough >= np.float32(ss["RoughnessThreshold"])).all()
    dq = torch.from_numpy(q.copy()).to(dev); dres = torch.zeros((len(steps), 12), dtype=torch.float32, device=dev)
    ctx.check(lib.pt_bsdf_sample(ctx.handle, C.c_void_p(dq.data_ptr()), len(steps), C.c_void_p(dres.data_ptr())))
    ctx.sync()
    res = dres.cpu().numpy()
    ok = res[:, 11].view(np.uint32) != 0
    throughputs = 0
    for k, (p, b) in enumerate(steps):
        e, vert = scatter[p, b], log[p, b]
        goes_bsdf = bool(ok[k]) and res[k, 3] != 0 and (res[k, 4:7] != 0).any()
        if b <= 3:
            assert bool(e["Goes"]) == goes_bsdf                          # (later bounces may also end by Russian roulette)
        if ok[k]:
            assert np.array_equal(e["L"].view(np.uint32), res[k, 0:3].view(np.uint32))          # the next direction, bit for bit
        if b <= 3 and goes_bsdf:
            thr = res[k, 4:7] * (np.float32(1.0) / res[k, 3])
            assert np.array_equal(vert["Throughput"].view(np.uint32), thr.view(np.uint32))
            throughputs += 1
    # Every vertex sees the next one: the probe is the kernel's own ray (GetSafeWorldRayOrigin, the sampled direction), ended 1e-4 above the
    # plane of the next vertex's face (its logged position and flat normal) -- a thousand fp32 roundings of a coordinate in this 2-unit room.
    # Nothing lies before a closest hit, so every probe is free. Cutting by a share of the distance to the logged position instead is not
    # sound at grazing incidence: the barycentrics of a sliver-projected triangle move the position along the face by more than that share.
    # A segment too short for the clearance (the next face closer than 1e-4 / cos) is left out and counted: at most 1 %.
    assert too_close <= 0.01 * len(rays), short                          # (path, bounce, distance along the ray to the next face, cosine there)
    rays = np.asarray(rays, np.float32)
    dr = torch.from_numpy(rays.copy()).to(dev); dv = torch.zeros((len(rays), 4), dtype=torch.float32, device=dev)
    ctx.check(lib.pt_trace_visibility(ctx.handle, C.c_void_p(dr.data_ptr()), len(rays), C.c_void_p(dv.data_ptr())))
    ctx.sync()
    vis = dv.cpu().numpy()
    print(f"log: {len(steps)} BSDF steps, {throughputs} throughputs, {len(rays)} segments, {too_close} too short, {int((vis[:, 3] != 1).sum())} occluded")
    assert more(throughputs, 500) and (vis[:, 3] == 1).all()


def test_log_validity(ptamd, pkg, rigs):
    _log_validity(ptamd, pkg, rigs, PINNED[0])


@pytest.mark.parametrize("pinned", RAGGED_PINNED, ids=_pinned_id)
def test_log_validity_ragged(ptamd, pkg, rigs, pinned):
    _log_validity(ptamd, pkg, rigs, pinned)


def test_query_decision(ptamd, pkg, rigs):
    rig, ref, scene, ss, out = _pinned_frames(ptamd, pkg, rigs)
    log = out[-1][0]
    hit = (log["Flags"] & R.HIT) != 0
    pos, nrm = log["Position"][hit], log["Normal"][hit]
    rng = np.random.default_rng(5)
    dist = np.exp(rng.uniform(np.log(0.01), np.log(8.0), len(pos))).astype(np.float32)
    rough = rng.uniform(0.0, 2.0, len(pos)).astype(np.float32)
    rough[::5] = 0.0                                                    # bounce 0: no footprint, never valid
    valid, rad, near = ref.query(np.array(scene.camera)["Position"], float(ss["SceneScale"]), pos, nrm, dist, rough)
    got = rig.r.sharc.debug_query(pos, nrm, dist, rough)
    ok = ~near
    print(f"query: {len(pos)} cases, {int(valid.sum())} valid, {int(near.sum())} within NEAR of a decision")
    assert near.mean() <= 0.01 and valid[ok].sum() > 100 and (~valid[ok]).sum() > 100
    assert np.array_equal(got["Valid"][ok] != 0, valid[ok])
    assert np.array_equal(got["Radiance"][ok].view(np.uint32), rad[ok].view(np.uint32))
    assert not (got["Valid"][::5] != 0).any()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------
def _region_means(img, gx=4, gy=4):
    H, W = img.shape[:2]
    lum = img[..., :3].astype(np.float64).mean(-1)
    return np.array([[lum[y * H // gy:(y + 1) * H // gy, x * W // gx:(x + 1) * W // gx].mean() for x in range(gx)] for y in range(gy)])


def test_end_to_end(ptamd, pkg, rigs):
    """Diffuse Cornell, static camera, 64 frames through the cache against the unchanged plain tracer averaged over the same frame indices
    at 16 spp. Figures are differences of region means (4 x 4 regions) and of the whole-image mean, relative to the yardstick's whole-image
    mean. The tolerance is twice the cache's measured offset plus the plain tracer's own spread (module constants)."""
    S, L = pkg.scenes, pkg.layouts
    W, H, N = 192, 108, 64
    scene = S.cornell_box(aspect=W / H, variant="diffuse")
    rig = Rig(ptamd, scene, W, H, capacity=1 << 18); rigs.append(rig)

    def mean_of(frames, spp, sharc=None):
        acc = np.zeros((H, W, 4), np.float64)
        for f in frames:
            acc += rig.frame(settings(pkg, W, H, spp=spp, frame=f), sharc=sharc)[1]
        return acc / len(frames)

    yard = mean_of(range(N), 16)
    other = mean_of(range(N, 2 * N), 16)
    cached = mean_of(range(N), 1, L.sharc_settings())
    assert np.isfinite(cached).all()
    scale = _region_means(yard, 1, 1)[0, 0]
    spread_r = np.abs(_region_means(other) - _region_means(yard)).max() / scale
    spread_i = abs(_region_means(other, 1, 1)[0, 0] - scale) / scale
    off_r = np.abs(_region_means(cached) - _region_means(yard)).max() / scale
    off_i = abs(_region_means(cached, 1, 1)[0, 0] - scale) / scale
    print(f"end to end: plain spread regions {spread_r:.4f} image {spread_i:.4f}; cache offset regions {off_r:.4f} image {off_i:.4f}; live entries {len(rig.map())}")
    assert off_r <= 2 * E2E_OFFSET_REGION + E2E_SPREAD_REGION
    assert off_i <= 2 * E2E_OFFSET_IMAGE + E2E_SPREAD_IMAGE


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------
def test_determinism(ptamd, pkg, rigs):
    S, L = pkg.scenes, pkg.layouts
    W, H = 160, 90
    scene = S.cornell_box(aspect=W / H, variant="ggx", glass_sphere=True)
    runs = []
    for _ in range(2):
        rig = Rig(ptamd, scene, W, H, capacity=1 << 18); rigs.append(rig)
        images = [rig.frame(settings(pkg, W, H, spp=2, frame=f), sharc=L.sharc_settings(downscale=2))[0] for f in range(8)]
        runs.append((images, rig.map()))
    assert len(runs[0][1]) > 1000 and runs[0][1] == runs[1][1]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------
def test_fewer_rays_once_warm(ptamd, pkg, rigs):
    """A C2-shaped frame (Cornell GGX, 4 spp, 8 bounces; a quarter of its 1920 x 1080 on each axis): from frame 8 on the cached frame traces
    strictly fewer secondary rays than the plain one, the update pass's own rays included."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 480, 270
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    rig = Rig(ptamd, scene, W, H, capacity=1 << 20); rigs.append(rig)
    for f in range(12):
        gs = settings(pkg, W, H, spp=4, frame=f)
        cached = rig.frame(gs, sharc=L.sharc_settings())[2][1]
        plain = rig.frame(gs)[2][1]
        print(f"frame {f}: secondary rays plain {plain} cached {cached} ({cached / plain:.3f})")
        if f >= 8:
            assert cached < plain


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------
def test_di_on(ptamd, pkg, rigs):
    """With an empty cache the DI-on query starts every sample's radiance with DI (Raytracing.hlsl:318), the plain frame adds DI once after
    the division. All terms are non-negative, so a chain of k roundings is within k * 2^-24 (relative, first order) of the exact value. A
    sample's radiance takes at most Bounces + 1 fused multiply-adds (one rounding each; emission or environment per vertex), plus the DI
    addition in the cached form; the sum over n samples n more, the division one, the plain form's DI addition one: chains of
    Bounces + n + 3 (cached) and Bounces + n + 3 (plain) roundings, so the two are at most (2 * Bounces + 2 * n + 6) * 2^-24 apart. The fp16
    Radiance may then round to the neighbouring value: one ulp."""
    S, L = pkg.scenes, pkg.layouts
    W, H, spp = 128, 72, 2
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    rig = Rig(ptamd, scene, W, H, flags=SKIP_UPDATE, denoiser_outputs=True); rigs.append(rig)
    gs = settings(pkg, W, H, spp=spp, frame=1, IsDIEnabled=1)
    plain = rig.frame(gs, di_samples=8)
    cached = rig.frame(gs, sharc=L.sharc_settings(), di_samples=8)
    a, b = plain[1][..., :3].astype(np.float64), cached[1][..., :3].astype(np.float64)
    assert (a > 0).mean() > 0.5
    assert (np.abs(a - b) <= (2 * int(gs["Bounces"]) + 2 * spp + 6) * 2.0 ** -24 * np.maximum(a, b)).all()
    ha, hb = plain[0][..., :3].astype(np.int64), cached[0][..., :3].astype(np.int64)
    assert np.abs(ha - hb).max() <= 1
    rig.ctx.set_debug_flags(0)                                          # and with the cache at work: finite frames
    for f in range(4):
        out = rig.frame(settings(pkg, W, H, spp=spp, frame=f, IsDIEnabled=1), sharc=L.sharc_settings(), di_samples=8)[1]
        assert np.isfinite(out).all() and out[..., :3].min() >= 0
    assert len(rig.map()) > 0


# ---- 10 ----------------------------------------------------------------------------------------------------------------------------
def test_errors_reset_and_viewer(ptamd, pkg, rigs):
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 36
    scene = S.cornell_box(aspect=W / H, variant="diffuse")
    rig = Rig(ptamd, scene, W, H, capacity=None, denoiser_outputs=True); rigs.append(rig)
    ctx, lib, sh = rig.ctx, rig.ctx.lib, rig.r.sharc
    gs = settings(pkg, W, H)
    rig.frame(gs)

    def refused(fn, text, kind=ptamd.PtInvalidArgument):
        with pytest.raises(kind) as e:
            fn()
        assert text in str(e.value), str(e.value)

    refused(lambda: rig.frame(gs, sharc=L.sharc_settings()), "pt_sharc_configure", ptamd.PtError)        # render before configure: NOT_READY (-2)
    refused(lambda: sh.Configure(1000), "multiple of 32")
    sh.Configure(1 << 14)

    def raw(**kw):
        s = L.sharc_settings().copy()
        for k, v in kw.items():
            s[k] = v
        return s

    rig.frame(gs, sharc=L.sharc_settings(downscale=2))
    before = len(rig.map())
    assert before > 0
    for kw, text in ((dict(DownscaleFactor=0), "DownscaleFactor"), (dict(DownscaleFactor=5), "DownscaleFactor"), (dict(SceneScale=4.0), "SceneScale"),
                     (dict(SceneScale=101.0), "SceneScale"), (dict(RoughnessThreshold=1.5), "RoughnessThreshold"), (dict(AccumulationFrames=0), "AccumulationFrames"),
                     (dict(AccumulationFrames=64), "AccumulationFrames"), (dict(MaxStaleFrames=0), "MaxStaleFrames"), (dict(MaxStaleFrames=256), "MaxStaleFrames"),
                     (dict(IsAntiFireflyEnabled=2), "IsAntiFireflyEnabled"), (dict(IsHashGridVisualizationEnabled=1), "visualisation")):
        s = raw(**kw)
        refused(lambda: ctx.check(lib.pt_sharc_set_constants(ctx.handle, C.c_void_p(s.ctypes.data))), text)
    t = ptamd._pack_textures(rig.r.textures)
    ctx.check(lib.pt_raytrace_render_sharc(ctx.handle, C.addressof(t)))                                   # a refused setting left downscale 2 active
    assert rig.r.sharc.download_update_paths().size == 0 and len(rig.map()) >= before
    for den in (L.DENOISER_NRD_REBLUR, L.DENOISER_NRD_RELAX):
        refused(lambda: rig.frame(settings(pkg, W, H, Denoiser=den), sharc=L.sharc_settings()), "NRD")
    rig.frame(settings(pkg, W, H, Denoiser=L.DENOISER_DLSS_RR), sharc=L.sharc_settings())                 # served
    ctx.set_sharding(0, 2, 16)
    refused(lambda: ctx.check(lib.pt_raytrace_render_sharc(ctx.handle, C.addressof(t))), "unsharded")
    ctx.set_sharding(0, 1, 16)
    ctx.set_debug_flags(0x2)
    refused(lambda: ctx.check(lib.pt_raytrace_render_sharc(ctx.handle, C.addressof(t))), "hit distance")
    ctx.set_debug_flags(0)
    refused(lambda: ctx.check(lib.pt_raytrace_render_sharc(ctx.handle, None)), "NULL")
    assert ctx.lib.pt_abi_version() == 4

    # a viewer of the scene has a cache of its own
    viewer = Rig(ptamd, None, W, H, capacity=1 << 14, shared_from=rig); rigs.append(viewer)
    assert len(viewer.map()) == 0 and len(rig.map()) > 0
    viewer.frame(gs, sharc=L.sharc_settings())
    assert len(viewer.map()) > 0
    sh.Reset()
    assert len(rig.map()) == 0 and len(viewer.map()) > 0                                                  # reset empties the map -- this context's


def test_demo_with_sharc():
    p = subprocess.run([DEMO, "--sharc", "--frames", "4", "--width", "320", "--height", "180", "--spp", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-600:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["sharc"] is True and line["sharc_entries"] > 0 and line["secondary_rays"] > 0
