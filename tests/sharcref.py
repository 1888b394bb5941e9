"""The SHARC radiance cache's rules ("Radiance cache") restated with numpy float32 / Python integer arithmetic: the
arbiter of tests/test_sharc_rules.py and tests/test_sharc_gpu.py. The hash map is a Python dict {key: [x, y, z, w]}: nothing observable
depends on the slot a key landed in. The SDK headers are not part of the reference tree, so these rules are the library's own, unpinned.

Grid   level = uint(clamp(0.5 * log2(|cam - p|^2), 1, 1023)); voxelSize = 2^level / SceneScale; cell = floor((p + 1e-4) / voxelSize) per axis;
       key = x:17 | y:17 | z:17 | level:10 | normal signs:3 (bit i set when n_i + 1e-3 < 0), from bit 0. Key 0 = empty.
Map    hash = J(lo32) ^ J(hi32), J = Jenkins' 32-bit integer hash; bucket base = (hash % capacity) / 32 * 32; 32 slots per bucket; a full
       bucket drops the sample (and ends the path).
Voxel  xyz = sums of radiance * 1e3 (u32); w = samples:18 | accumulated frames:6 << 18 | stale frames:8 << 24. A deposit is
       uint(min(c * 1e3f, 16383)) per component, 0 for a non-finite or non-positive c: 2^18 deposits cannot wrap a sum. In this frame's
       buffer w counts the frame's samples in all 32 bits.
"""
import numpy as np

F = np.float32
POSITION_BIAS, NORMAL_BIAS, RADIANCE_SCALE = F(1e-4), F(1e-3), F(1e3)
BUCKET = 32
SAMPLE_BITS, FRAME_BITS = 18, 6
SAMPLE_MASK, FRAME_MASK = (1 << SAMPLE_BITS) - 1, (1 << FRAME_BITS) - 1
SAMPLE_CAP = 1 << 17
DEPOSIT_MAX = F(16383.0)
FIREFLY_FACTOR = 8
SQRT3 = F(1.7320508)
HIT, MISS, ENDED, RESAMPLED = 1, 2, 4, 8
NEAR = 1e-5                      # the relative margin inside which a decision is left out of an exact comparison


def jenkins(a):
    a &= 0xFFFFFFFF
    a = ((a + 0x7ED55D16) + (a << 12)) & 0xFFFFFFFF
    a = ((a ^ 0xC761C23C) ^ (a >> 19)) & 0xFFFFFFFF
    a = ((a + 0x165667B1) + (a << 5)) & 0xFFFFFFFF
    a = ((a + 0xD3A2646C) ^ (a << 9)) & 0xFFFFFFFF
    a = ((a + 0xFD7046C5) + (a << 3)) & 0xFFFFFFFF
    a = ((a ^ 0xB55A4F09) ^ (a >> 16)) & 0xFFFFFFFF
    return a


def key_hash(key):
    return jenkins(key & 0xFFFFFFFF) ^ jenkins(key >> 32)


def bucket(key, capacity):
    return (key_hash(key) % capacity) // BUCKET * BUCKET


def grid(cam, pos, nrm, scene_scale):
    """(keys uint64, levels, voxel sizes float32, near) of points (n, 3) with normals. near[i]: the point sits within NEAR (relative) of a
    level boundary, a cell face or a normal-sign threshold, where one ulp of log2 or of the division decides."""
    cam = np.asarray(cam, F).reshape(3); p = np.asarray(pos, F).reshape(-1, 3); n = np.asarray(nrm, F).reshape(-1, 3)
    d = cam[None, :] - p
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(divide="ignore"):
        lg = F(0.5) * np.log2(d2).astype(F)
    lv = np.minimum(np.maximum(lg, F(1.0)), F(1023.0))
    lv = np.where(np.isnan(lv), F(1.0), lv)
    level = lv.astype(np.uint32)
    size = (np.ldexp(F(1.0), level.astype(np.int32)).astype(F) / F(scene_scale)).astype(F)
    q = ((p + POSITION_BIAS) / size[:, None]).astype(F)
    cell = np.floor(q).astype(np.int64)
    bits = ((n[:, 0] + NORMAL_BIAS < 0).astype(np.uint64) | ((n[:, 1] + NORMAL_BIAS < 0).astype(np.uint64) << np.uint64(1))
            | ((n[:, 2] + NORMAL_BIAS < 0).astype(np.uint64) << np.uint64(2)))
    c = (cell & 0x1FFFF).astype(np.uint64)
    keys = c[:, 0] | (c[:, 1] << np.uint64(17)) | (c[:, 2] << np.uint64(34)) | (level.astype(np.uint64) << np.uint64(51)) | (bits << np.uint64(61))
    lg64 = 0.5 * np.log2(np.maximum(d2.astype(np.float64), 1e-300))
    near = (np.abs(lg64 - np.round(lg64)) < NEAR * np.maximum(1.0, np.abs(lg64))) & (lg64 > 0.5)
    q64 = q.astype(np.float64)
    near |= (np.abs(q64 - np.round(q64)) < NEAR * np.maximum(1.0, np.abs(q64))).any(1)
    near |= (np.abs(n.astype(np.float64) + 1e-3) < NEAR).any(1)
    return keys, level, size, near


def unpack(w):
    return w & SAMPLE_MASK, (w >> SAMPLE_BITS) & FRAME_MASK, w >> (SAMPLE_BITS + FRAME_BITS)


def pack(samples, frames, stale):
    return samples | (frames << SAMPLE_BITS) | (stale << (SAMPLE_BITS + FRAME_BITS))


def deposit_word(c):
    c = F(c)
    if not (np.isfinite(c) and c > 0):
        return 0
    return int(min(F(c * RADIANCE_SCALE), DEPOSIT_MAX))


def voxel_radiance(v):
    d = F(F(v[3] & SAMPLE_MASK) * RADIANCE_SCALE)
    return np.array([F(v[0]) / d, F(v[1]) / d, F(v[2]) / d], F)


class Cache:
    """The map and the two voxel buffers: `current` holds this frame's deposits, `resolved` the history (PreviousVoxelData during the update,
    the resolved buffer after resolve())."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.keys = set()                 # HashEntries
        self.current = {}
        self.resolved = {}
        self.refused = 0                  # inserts a full bucket turned away

    def fullest_bucket(self):
        n = {}
        for k in self.keys:
            b = bucket(k, self.capacity); n[b] = n.get(b, 0) + 1
        return max(n.values()) if n else 0

    def insert(self, key):
        if key in self.keys:
            return True
        b = bucket(key, self.capacity)
        if sum(1 for k in self.keys if bucket(k, self.capacity) == b) >= BUCKET:
            self.refused += 1
            return False
        self.keys.add(key)
        return True

    def deposit(self, key, c, samples):
        v = self.current.setdefault(key, [0, 0, 0, 0])
        for i in range(3):
            v[i] = (v[i] + deposit_word(c[i])) & 0xFFFFFFFF
        v[3] += samples

    # ---- update: one path's vertex log through the SharcState machine --------------------------------------------------------------
    def update_path(self, vertices, keys=None):
        """vertices: the (bounces,) log entries of one path (layouts.SHARC_PATH_VERTEX); keys: their keys (default: the logged ones).
        Returns the number of resampled terminations."""
        idx, weight, length, resampled = [None] * 4, [np.zeros(3, F)] * 4, 0, 0
        for b, e in enumerate(vertices):
            flags = int(e["Flags"])
            if flags == 0:
                break
            rad = np.asarray(e["Radiance"], F)
            if flags & MISS:
                for i in range(length):
                    self.deposit(idx[i], (rad * weight[i]).astype(F), 0)
                break
            key = int(keys[b]) if keys is not None else int(e["KeyLo"]) | (int(e["KeyHi"]) << 32)
            if not self.insert(key):
                break
            depth = int(np.floor(F(F(F(1.0) + F(2.0) * F(e["Random"])) + F(0.5))))
            value, took = rad, False
            if depth <= length:
                h = self.resolved.get(key)
                if h is not None and (h[3] & SAMPLE_MASK):
                    value, took = voxel_radiance(h), True
            if not took:
                self.deposit(key, value, 1)
            for i in range(length):
                self.deposit(idx[i], (value * weight[i]).astype(F), 0)
            if took:
                resampled += 1
                break
            idx = [key] + idx[:3]; weight = [np.ones(3, F)] + weight[:3]
            length = min(length + 1, 3)
            if flags & ENDED:
                break
            t = np.asarray(e["Throughput"], F)
            for i in range(length):
                weight[i] = (weight[i] * t).astype(F)
        return resampled

    # ---- resolve ----------------------------------------------------------------------------------------------------------------------
    def resolve(self, accumulation_frames=10, max_stale_frames=64, anti_firefly=True):
        stale_limit = min(max(max_stale_frames, 8), 255)
        out = {}
        for key in list(self.keys):
            c = list(self.current.get(key, [0, 0, 0, 0])); p = self.resolved.get(key, [0, 0, 0, 0])
            v = resolve_voxel(c, p, accumulation_frames, stale_limit, anti_firefly)
            if v is None:
                self.keys.discard(key)
            else:
                out[key] = v
        self.resolved, self.current = out, {}

    def query(self, cam, scene_scale, pos, nrm, distance, previous_roughness):
        """(valid, radiance, near) per point: the query decision against the resolved buffer."""
        keys, level, size, near = grid(cam, pos, nrm, scene_scale)
        dist = np.asarray(distance, F).reshape(-1); pr = np.asarray(previous_roughness, F).reshape(-1)
        t1 = (size * SQRT3).astype(F)
        r = np.minimum(pr, F(0.99)); alpha = (r * r).astype(F); a2 = (alpha * alpha).astype(F)
        foot = (dist * np.sqrt((F(0.5) * a2 / (F(1.0) - a2)).astype(F)).astype(F)).astype(F)
        ok = (dist > t1) & (foot > size)
        near = near | (np.abs(dist.astype(np.float64) - t1) < NEAR * t1) | (np.abs(foot.astype(np.float64) - size) < NEAR * size)
        valid = np.zeros(len(keys), bool); rad = np.zeros((len(keys), 3), F)
        for i, k in enumerate(keys):
            v = self.resolved.get(int(k))
            if ok[i] and v is not None and (v[3] & SAMPLE_MASK):
                valid[i], rad[i] = True, voxel_radiance(v)
        return valid, rad, near


def f32(n):
    """float(u64) with ONE rounding to nearest even (through a double a 64-bit integer would round twice)"""
    if n < (1 << 53):
        return F(n)
    k = n.bit_length() - 40
    m = (n >> k) | (1 if n & ((1 << k) - 1) else 0)      # 40 leading bits, the rest as a sticky bit
    return F(np.ldexp(np.float64(m), k))


def _scale(value, s):
    return int(F(f32(value) * s))        # the product is fp32, the conversion truncates


def resolve_voxel(c, p, accumulation_frames, stale_limit, anti_firefly):
    """this frame's word c (w = samples) and the history p -> the resolved word, or None when the voxel is evicted"""
    cN = min(c[3], 1 << SAMPLE_BITS); pN, pF, pS = unpack(p[3])      # a frame counts at most 2^18 samples of a voxel
    c = list(c)
    if anti_firefly and cN and pN:
        lc = 77 * c[0] + 150 * c[1] + 29 * c[2]; lh = 77 * p[0] + 150 * p[1] + 29 * p[2]
        lim, got = FIREFLY_FACTOR * lh * cN, lc * pN
        if lh and got > lim:
            s = F(f32(lim) / f32(got))
            c[:3] = [_scale(x, s) for x in c[:3]]
    R = [c[i] + p[i] for i in range(3)]; N = cN + pN; Fr = pF + 1
    # a rescale truncates the sample count; the sums follow the count it actually got (new / old), so the voxel's mean is kept
    if Fr > accumulation_frames:
        Nn = _scale(N, F(F(accumulation_frames) / F(Fr)))
        s = F(f32(Nn) / f32(N)) if N else F(0.0)
        R = [_scale(x, s) for x in R]; N = Nn; Fr = accumulation_frames
    if N > SAMPLE_CAP:
        Nn = _scale(N, F(F(SAMPLE_CAP) / f32(N)))
        s = F(f32(Nn) / f32(N))
        R = [_scale(x, s) for x in R]; N = Nn
    S = 0 if cN else pS + 1
    if S >= stale_limit:
        return None
    return [min(x, 0xFFFFFFFF) for x in R] + [pack(N, Fr, S)]
