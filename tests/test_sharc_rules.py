"""The SHARC radiance cache's rules without a GPU: settings and layouts, the exported symbols, and the restatement tests/sharcref.py held
to known answers (computed once from the rules of DESIGN.md section 1, "Radiance cache", and pinned) and to the behaviours the resolve
pass promises."""
import numpy as np
import pytest

import sharcref as R

SHARC_EXPORTS = ["pt_sharc_configure", "pt_sharc_set_constants", "pt_raytrace_render_sharc", "pt_sharc_reset", "pt_sharc_download",
                 "pt_sharc_debug_keys", "pt_sharc_debug_query", "pt_sharc_download_update_paths", "pt_sharc_download_update_scatter"]


def test_defaults_are_the_references(pkg):
    L = pkg.layouts
    s = L.sharc_settings()
    assert int(s["DownscaleFactor"]) == 4 and float(s["SceneScale"]) == 50.0 and float(s["RoughnessThreshold"]) == np.float32(0.4)
    assert int(s["AccumulationFrames"]) == 10 and int(s["MaxStaleFrames"]) == 64
    assert int(s["IsAntiFireflyEnabled"]) == 1 and int(s["IsHashGridVisualizationEnabled"]) == 0
    assert L.SHARC_DEFAULT_CAPACITY == 1 << 22 and L.SHARC_DEFAULT_CAPACITY % R.BUCKET == 0


def test_struct_sizes(pkg):
    L = pkg.layouts
    assert L.SHARC_SETTINGS.itemsize == 28 and L.SHARC_ENTRY.itemsize == 32
    assert L.SHARC_QUERY_RESULT.itemsize == 16 and L.SHARC_PATH_VERTEX.itemsize == 64 and L.SHARC_PATH_SCATTER.itemsize == 128
    assert L.GRAPHICS_SETTINGS.itemsize == 80                       # PtGraphicsSettings keeps its size: the cache has calls of its own
    assert (L.SHARC_VERTEX_HIT, L.SHARC_VERTEX_MISS, L.SHARC_VERTEX_ENDED, L.SHARC_VERTEX_RESAMPLED) == (R.HIT, R.MISS, R.ENDED, R.RESAMPLED)


@pytest.mark.parametrize("kw", [dict(downscale=0), dict(downscale=5), dict(scene_scale=4.9), dict(scene_scale=100.5), dict(roughness_threshold=-0.1),
                                dict(roughness_threshold=1.1), dict(accumulation_frames=0), dict(accumulation_frames=64), dict(max_stale_frames=0),
                                dict(max_stale_frames=256), dict(visualization=True)])
def test_settings_out_of_range_are_refused(pkg, kw):
    with pytest.raises(ValueError):
        pkg.layouts.sharc_settings(**kw)


def test_symbols_are_exported(ptamd):
    lib = ptamd.load_library()
    for s in SHARC_EXPORTS:
        assert s in ptamd.EXPORTS and hasattr(lib, s), s
    assert lib.pt_abi_version() == 4


def test_key_and_hash_known_answers():
    assert [R.jenkins(v) for v in (0, 1, 0xDEADBEEF)] == [0x6B4ED927, 0xB48681B6, 0x7FF0EADA]
    cam = [0.5, -0.25, -1.95]
    pos = np.array([[0.3, -0.7, 0.9], [-1.0, 1.0, 1.0], [10.5, 3.25, -7.75], [0, 0, 0]], np.float32)
    nrm = np.array([[0, 1, 0], [-1, 0, 0], [0.5, -0.5, -0.7], [-0.0005, 0, -0.002]], np.float32)
    keys, level, size, near = R.grid(cam, pos, nrm, 50.0)
    assert [int(k) for k in keys] == [0x8005BFFDC0007, 0x200800640033FFE7, 0xC01FFF3C00280041, 0x8008000000000000]
    assert level.tolist() == [1, 1, 3, 1] and size.tolist() == [np.float32(0.04), np.float32(0.04), np.float32(0.16), np.float32(0.04)]
    assert not near.any()
    assert [R.key_hash(int(k)) for k in keys] == [0x3A437819, 0x851C7E7B, 0xB2EC2394, 0xC427B37E]
    assert [R.bucket(int(k), 1 << 22) for k in keys] == [227328, 1867360, 2892672, 2601824]
    # the fields, one by one: a negative cell keeps its low 17 bits, the level sits at bit 51, the normal signs at bit 61
    k = int(keys[1])
    assert k & 0x1FFFF == (-25) & 0x1FFFF and (k >> 17) & 0x1FFFF == 25 and (k >> 34) & 0x1FFFF == 25 and (k >> 51) & 0x3FF == 1 and k >> 61 == 1
    assert all(int(k) != 0 for k in keys)                           # level >= 1: no key is the empty marker


def test_near_flags_the_decisions_an_ulp_can_turn():
    cam = [0, 0, 0]
    pos = np.array([[2.0, 0, 0], [0.08 - 1e-4, 0.5, 0.5], [0.5, 0.5, 0.5]], np.float32)      # |p| = 2: level boundary; x on a cell face
    nrm = np.array([[0, 1, 0], [0, 1, 0], [-1e-3, 1, 0]], np.float32)                         # n_x on the sign threshold
    near = R.grid(cam, pos, nrm, 50.0)[3]
    assert near.tolist() == [True, True, True]


def _frames(deposit, n, **kw):
    c = R.Cache(1 << 10); key = 0x8000000000001
    for _ in range(n):
        assert c.insert(key)
        for d in deposit:
            c.deposit(key, d, 1)
        c.resolve(**kw)
    return c.resolved.get(key)


def test_constant_deposits_converge_to_their_mean():
    v = _frames([(0.5, 0.25, 2.0)] * 7, 40)
    samples, frames, stale = R.unpack(v[3])
    assert frames == 10 and stale == 0 and 0 < samples <= 70
    assert np.allclose(R.voxel_radiance(v), [0.5, 0.25, 2.0], rtol=2e-3)     # truncation of the rescales: below 1 / samples
    mixed = _frames([(1.0, 1.0, 1.0), (3.0, 3.0, 3.0)], 40)
    assert np.allclose(R.voxel_radiance(mixed), [2.0, 2.0, 2.0], rtol=2e-3)


def test_accumulation_frames_rescale():
    # frames 1..10 add up; frame 11 scales the samples by 10 / 11, truncating, the sums by the ratio the samples got, and holds the frame count at 10
    c = R.Cache(1 << 10); key = 0x8000000000001
    for f in range(1, 12):
        c.insert(key); c.deposit(key, (1.0, 1.0, 1.0), 1); c.resolve()
        v = c.resolved[key]
        if f <= 10:
            assert v == [1000 * f] * 3 + [R.pack(f, f, 0)]
    n = int(np.float32(np.float32(11) * np.float32(np.float32(10) / np.float32(11))))
    assert n == 10 and v == [int(np.float32(np.float32(11000) * np.float32(np.float32(n) / np.float32(11))))] * 3 + [R.pack(n, 10, 0)]
    assert np.allclose(R.voxel_radiance(v), 1.0, rtol=1e-6)
    # the mean survives the truncation of a small count: 5 samples -> 4, and a count that reaches 0 takes its sums along
    assert R.resolve_voxel([0, 0, 0, 0], [5000, 2500, 0, R.pack(5, 10, 0)], 10, 64, False) == [4000, 2000, 0, R.pack(4, 10, 1)]
    assert R.resolve_voxel([0, 0, 0, 0], [900, 900, 900, R.pack(1, 10, 0)], 10, 64, False) == [0, 0, 0, R.pack(0, 10, 1)]


def test_sample_cap_rescale():
    p = [5 * 10 ** 8, 0, 7, R.pack(R.SAMPLE_CAP, 3, 0)]
    v = R.resolve_voxel([10 ** 6, 0, 1, 1000], p, 10, 64, False)
    n0 = np.float32(R.SAMPLE_CAP + 1000)
    n1 = int(np.float32(n0 * np.float32(np.float32(R.SAMPLE_CAP) / n0)))
    s = np.float32(np.float32(n1) / n0)
    assert v[0] == int(np.float32(np.float32(5 * 10 ** 8 + 10 ** 6) * s)) and v[1] == 0 and v[2] == int(np.float32(np.float32(8) * s))
    samples, frames, stale = R.unpack(v[3])
    assert samples == n1 and R.SAMPLE_CAP - 1 <= n1 <= R.SAMPLE_CAP and frames == 4 and stale == 0


def test_eviction_at_max_stale_frames():
    for limit, expect in ((64, 64), (3, 8), (255, 255)):          # max(MaxStaleFrames, 8), at most 255
        c = R.Cache(1 << 10); key = 0x8000000000001
        c.insert(key); c.deposit(key, (1, 1, 1), 1); c.resolve(max_stale_frames=limit)
        for f in range(1, expect):
            c.resolve(max_stale_frames=limit)
            assert key in c.keys and R.unpack(c.resolved[key][3])[2] == f
        c.resolve(max_stale_frames=limit)
        assert key not in c.keys and key not in c.resolved
    # a sample resets the count
    c = R.Cache(1 << 10); c.insert(key); c.deposit(key, (1, 1, 1), 1); c.resolve()
    for _ in range(5):
        c.resolve()
    c.deposit(key, (1, 1, 1), 1); c.resolve()
    assert R.unpack(c.resolved[key][3])[2] == 0


def test_deposit_clamp_and_no_wrap():
    assert R.deposit_word(np.float32(1e9)) == 16383 and R.deposit_word(np.float32(16.3835)) == 16383
    assert R.deposit_word(np.float32(2.5)) == 2500 and R.deposit_word(np.float32(0.0004)) == 0
    for bad in (np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(-1.0), np.float32(0.0)):
        assert R.deposit_word(bad) == 0
    # 2^18 deposits of the largest word stay below 2^32 ...
    assert (1 << 18) * 16383 < 1 << 32
    # ... and the resolve adds in 64 bits and saturates: a full history (2^17 samples at the clamp) plus such a frame never wraps
    p = [0xFFFFFFFF, R.SAMPLE_CAP * 16383, 0, R.pack(R.SAMPLE_CAP, 10, 0)]
    cfr = [(1 << 18) * 16383 - 5, (1 << 17) * 16383, 3, 1 << 17]
    v = R.resolve_voxel(cfr, p, 10, 64, False)
    for k in range(3):
        exact = (cfr[k] + p[k]) * (10 / 11) * (R.SAMPLE_CAP / ((cfr[3] + R.SAMPLE_CAP) * 10 / 11))
        assert v[k] <= 0xFFFFFFFF and abs(v[k] - min(exact, 0xFFFFFFFF)) <= 1e-4 * max(exact, 1) + 2
    v = R.resolve_voxel([0xFFFFFFFF, 0, 0, 1], [0xFFFFFFFF, 0, 0, R.pack(1, 1, 0)], 10, 64, False)
    assert v[0] == 0xFFFFFFFF                                       # saturated, not wrapped


def test_anti_firefly_clamps_against_the_history_but_lets_new_light_in():
    hist = [1000 * 100, 1000 * 100, 1000 * 100, R.pack(100, 5, 0)]                 # mean 1.0 over 100 samples
    spike = [16383 * 4, 16383 * 4, 16383 * 4, 4]                                     # mean 16.383 over 4 samples
    off = R.resolve_voxel(spike, hist, 10, 64, False)
    on = R.resolve_voxel(spike, hist, 10, 64, True)
    assert off[0] == 100000 + 16383 * 4
    assert abs(on[0] - (100000 + 8 * 1000 * 4)) <= 2 and on[3] == off[3]             # the frame's mean is held to 8 x the history's
    mild = [3000 * 4, 3000 * 4, 3000 * 4, 4]                                         # below the limit: untouched
    assert R.resolve_voxel(mild, hist, 10, 64, True) == R.resolve_voxel(mild, hist, 10, 64, False)
    # an empty or all-zero history clamps nothing: a newly lit voxel converges
    for dark in ([0, 0, 0, 0], [0, 0, 0, R.pack(500, 10, 0)]):
        assert R.resolve_voxel(spike, dark, 10, 64, True) == R.resolve_voxel(spike, dark, 10, 64, False)
    c = R.Cache(1 << 10); key = 0x8000000000001
    c.insert(key)
    for _ in range(12):                                                              # 12 dark frames, then the light comes on
        c.deposit(key, (0.0, 0.0, 0.0), 4); c.resolve()
    for _ in range(120):                                                             # (the dark samples leave the history by 10 / 11 per frame)
        for _ in range(4):
            c.deposit(key, (5.0, 5.0, 5.0), 1)
        c.resolve()
    assert np.allclose(R.voxel_radiance(c.resolved[key]), [5.0, 5.0, 5.0], rtol=5e-3)


def test_update_state_machine_propagates_and_resamples():
    V = np.dtype({"names": ["Position", "Flags", "Normal", "Random", "Radiance", "KeyLo", "Throughput", "KeyHi"],
                  "formats": [("<f4", 3), "<u4", ("<f4", 3), "<f4", ("<f4", 3), "<u4", ("<f4", 3), "<u4"], "offsets": [0, 12, 16, 28, 32, 44, 48, 60], "itemsize": 64})
    path = np.zeros(4, V)
    ka, kb, kc = 0x8000000000001, 0x8000000000002, 0x8000000000003
    path["Flags"] = [R.HIT, R.HIT, R.HIT, R.MISS | R.ENDED]
    path["Radiance"] = [(0, 0, 0), (0, 0, 0), (2, 2, 2), (1, 1, 1)]
    path["Throughput"] = [(0.5, 0.5, 0.5), (0.5, 0.25, 1.0), (1, 1, 1), (0, 0, 0)]
    path["Random"] = [0.9, 0.9, 0.9, 0]
    c = R.Cache(1 << 10)
    assert c.update_path(path, [ka, kb, kc, 0]) == 0
    # vertex c deposits 2 into itself, 2 * (0.5, 0.25, 1) into b and 2 * (0.5, 0.25, 1) * 0.5 into a; the miss adds 1 * the weights
    assert c.current[kc] == [2000 + 1000, 2000 + 1000, 2000 + 1000, 1]
    assert c.current[kb] == [1000 + 500, 500 + 250, 2000 + 1000, 1]
    assert c.current[ka] == [500 + 250, 250 + 125, 1000 + 500, 1]
    c.resolve()
    # next frame: depth = round(1 + 2 * 0.1) = 1 <= pathLength at the second vertex, whose voxel has history: the path ends there
    path["Random"] = [0.1, 0.1, 0.1, 0]
    assert c.update_path(path, [ka, kb, kc, 0]) == 1
    hb = R.voxel_radiance(c.resolved[kb])
    assert c.current[ka] == [int(np.float32(hb[i] * np.float32(0.5)) * np.float32(1000)) for i in range(3)] + [1]
    assert kb not in c.current and kc not in c.current
