"""Restatement of the local-light sampling rules of the DI pass ("Local-light sampling"): the power prefix sum and
its selection rule, Power_RIS presampling, TriangleLight::CalculateWeightForVolume, the ReGIR build, the screen-tile and cell choice and
the Uniform / Power_RIS / ReGIR candidates of initial sampling. Each step the device computes in float32 with a discrete outcome is
restated with the same float32 steps (vectorised over entries); p-hat at a surface comes from restirref.target_pdfs (float64)."""
import numpy as np

import restirref as R

M32 = 0xFFFFFFFF
SALT_PRESAMPLE, SALT_REGIR, SALT_REGIR_COHERENT, SALT_SCREEN_TILE = 0x44490004, 0x44490005, 0x44490006, 0x44490007
TILE_COUNT, TILE_SIZE = 128, 1024                   # the RTXDI SDK's defaults (unpinned)
SCREEN_TILE = 16
GRID, CELL_LIGHTS = 16, 512
JITTER_SCALE = 2.0                                  # max(0, 2 * samplingJitter), jitter 1
SCAN_BLOCK = 1024
LUMA32 = np.array([0.2990, 0.5870, 0.1140], np.float32)
f32 = np.float32


# ---- vectorised RNG (restirref.Rng over uint64 arrays) -------------------------------------------------------------------------
def _hash(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32; x ^= x >> 15; x = (x * 0x846CA68B) & M32; x ^= x >> 16
    return x


def rng_states(px, py, frame, salt):
    px, py = np.asarray(px, np.uint64), np.asarray(py, np.uint64)
    seed = _hash(np.uint64(frame + 0x035F9F29))
    v = ((px << np.uint64(16)) | (py & np.uint64(0xFFFF))) & M32
    st = seed ^ ((_hash(v) + 0x9E3779B9 + ((seed << np.uint64(6)) & M32) + (seed >> np.uint64(2))) & M32)
    return _hash(st ^ np.uint64(salt))


def rng_next(state):
    """(new state, float32 draws)"""
    state = (state * 1664525 + 1013904223) & M32
    return state, (_hash(state) >> np.uint64(8)).astype(np.float32) * f32(1.0 / 16777216.0)


def index_of(u, n):
    """min(uint(u * n), n - 1) in float32"""
    return np.minimum((np.asarray(u, np.float32) * f32(n)).astype(np.int64), n - 1)


# ---- the power prefix sum (k_cdf_local / k_cdf_blocks / k_cdf_add) and select_light ------------------------------------------------
def power_cdf(power):
    """the device's inclusive prefix sum, float32, in its order; returns (cdf, total)"""
    power = np.asarray(power, np.float32)
    n = len(power)
    nb = (n + SCAN_BLOCK - 1) // SCAN_BLOCK
    p = np.zeros(nb * SCAN_BLOCK, np.float32); p[:n] = power
    v = p.reshape(nb, 256, 4).copy()
    for j in range(1, 4):
        v[:, :, j] = v[:, :, j - 1] + v[:, :, j]
    part = v[:, :, 3].copy()
    off = 1
    while off < 256:
        part = np.concatenate([part[:, :off], part[:, off:] + part[:, :-off]], 1)
        off <<= 1
    before = np.concatenate([np.zeros((nb, 1), np.float32), part[:, :-1]], 1)
    local = (before[:, :, None] + v).reshape(-1)[:n]
    sums = part[:, 255]
    offs, s = np.zeros(nb, np.float32), f32(0)
    for b in range(nb):
        offs[b] = s; s = f32(s + sums[b])
    cdf = local.copy()
    k = np.arange(n)
    hi = k >= SCAN_BLOCK
    cdf[hi] = offs[k[hi] // SCAN_BLOCK] + local[hi]
    cdf[n - 1] = s
    return cdf, s


def select_light(cdf, x, total, ge_rule=True):
    """first light whose prefix exceeds x; x >= total: the first that reaches the total (ge_rule=False drops that rule: a mutation)"""
    x = np.asarray(x, np.float32)
    i = np.searchsorted(cdf, x, side="right")
    if ge_rule:
        i = np.where(x < total, i, np.searchsorted(cdf, total, side="left"))
    return i


# ---- Power_RIS presampling ---------------------------------------------------------------------------------------------------------
def presample_tiles(power, frame, ge_rule=True):
    """k_di_presample_tiles: (LightIndex int64 [128 * 1024], InvSourcePdf float32); -1 / 0 when the total is not positive"""
    power = np.asarray(power, np.float32)
    cdf, total = power_cdf(power)
    g = np.arange(TILE_COUNT * TILE_SIZE, dtype=np.uint64)
    if not (total > 0 and np.isfinite(total)):
        return np.full(len(g), -1, np.int64), np.zeros(len(g), np.float32)
    _, u = rng_next(rng_states(g & np.uint64(0xFFF), g >> np.uint64(12), frame, SALT_PRESAMPLE))
    li = select_light(cdf, u * total, total, ge_rule)
    li = np.minimum(li, len(power) - 1)
    return li, (total / power[li]).astype(np.float32)


# ---- CalculateWeightForVolume ------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _dot32(a, b):
    """sop3: a.x b.x rounded, then two fused multiply-adds"""
    return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(np.float32)))


def volume_weight32(lights, li, centre, radius, two_sided=False):
    """di_volume_weight in float32, the kernel's order. lights: TRIANGLE_LIGHT records; li, centre [.., 3], radius: broadcastable"""
    lt = lights[li]
    base, e0, e1, nrm = (lt[k].astype(np.float32) for k in ("Base", "Edge0", "Edge1", "Normal"))
    c = np.asarray(centre, np.float32)
    radius = np.asarray(radius, np.float32)
    d = _dot32((c - base).astype(np.float32), nrm)
    cull = (np.abs(d) > radius) if two_sided else (d < -radius)
    mid = (base + ((e0 + e1).astype(np.float32) / f32(3.0)).astype(np.float32)).astype(np.float32) - c
    dc = np.sqrt(_dot32(mid, mid)).astype(np.float32)
    value = (dc + (radius * f32(1.1547)).astype(np.float32)).astype(np.float32)
    dist = (dc + ((radius * radius * radius).astype(np.float32) / (value * value).astype(np.float32)).astype(np.float32)).astype(np.float32)
    sa = np.minimum((lt["Area"].astype(np.float32) / (dist * dist).astype(np.float32)).astype(np.float32), f32(2.0) * f32(np.pi))
    lum = _dot32(lt["Radiance"].astype(np.float32), np.broadcast_to(LUMA32, lt["Radiance"].shape))
    return np.where(cull, f32(0), (sa * lum).astype(np.float32)).astype(np.float32)


def volume_weight64(base, e0, e1, radiance, centre, radius):
    """Light.hlsli:16-24, 84-95 in float64 (TriangleLight::Initialize for the normal and area)"""
    base, e0, e1, radiance, c = (np.asarray(v, np.float64) for v in (base, e0, e1, radiance, centre))
    n = np.cross(e0, e1)
    ln = np.linalg.norm(n)
    nrm, area = (n / ln, ln / 2) if ln > 0 else (np.zeros(3), 0.0)
    if np.dot(c - base, nrm) < -radius:
        return 0.0
    dc = np.linalg.norm(base + (e0 + e1) / 3 - c)
    value = dc + radius * 1.1547
    dist = dc + radius ** 3 / value ** 2
    return min(area / dist ** 2, 2 * np.pi) * float(np.dot(radiance, [0.2990, 0.5870, 0.1140]))


# ---- ReGIR ---------------------------------------------------------------------------------------------------------------------------
def cell_centre(cells, centre, cell_size):
    """cells: flat cell indices (x fastest) -> float32 centres: centre + (i - 7.5) * size per axis"""
    cells = np.asarray(cells, np.int64)
    ijk = np.stack([cells % GRID, (cells // GRID) % GRID, cells // (GRID * GRID)], -1).astype(np.float32)
    h = f32(GRID // 2) - f32(0.5)
    cs = f32(cell_size)
    return (np.asarray(centre, np.float32) + ((ijk - h) * cs).astype(np.float32)).astype(np.float32)


def cell_radius(cell_size):
    return f32(f32(0.5) * np.sqrt(f32(3.0))) * f32(cell_size)


def regir_build(lights, tiles_li, tiles_inv, cells, centre, cell_size, build_samples, frame, store_build_samples=True, two_sided=False):
    """k_di_regir_build for every slot of the given cells: (LightIndex int64 [len(cells), 512], weight float32); -1 / 0 = empty"""
    cells = np.asarray(cells, np.int64)
    g = (cells[:, None] * CELL_LIGHTS + np.arange(CELL_LIGHTS)[None, :]).reshape(-1).astype(np.uint64)
    c = np.repeat(cell_centre(cells, centre, cell_size), CELL_LIGHTS, 0)
    radius = cell_radius(cell_size)
    rng = rng_states(g & np.uint64(0xFFF), g >> np.uint64(12), frame, SALT_REGIR)
    _, ct = rng_next(rng_states(g >> np.uint64(8), np.zeros_like(g), frame, SALT_REGIR_COHERENT))
    tile = index_of(ct, TILE_COUNT)
    wsum = np.zeros(len(g), np.float32); psel = np.zeros(len(g), np.float32); sel = np.full(len(g), -1, np.int64)
    for _ in range(build_samples):
        rng, u = rng_next(rng)
        rng, r = rng_next(rng)
        e = tile * TILE_SIZE + index_of(u, TILE_SIZE)
        li, inv = tiles_li[e], tiles_inv[e].astype(np.float32)
        ok = li >= 0
        p = np.where(ok, volume_weight32(lights, np.where(ok, li, 0), c, radius, two_sided), f32(0)).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(p > 0, (p / (f32(1.0) / inv).astype(np.float32)).astype(np.float32), f32(0)).astype(np.float32)
        wsum = (wsum + w).astype(np.float32)
        take = (r * wsum).astype(np.float32) < w
        sel = np.where(take, li, sel); psel = np.where(take, p, psel)
    m = f32(build_samples) if store_build_samples else f32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        wt = np.where(psel > 0, (wsum / (psel * m).astype(np.float32)).astype(np.float32), f32(0)).astype(np.float32)
    return np.where(psel > 0, sel, -1).reshape(len(cells), CELL_LIGHTS), wt.reshape(len(cells), CELL_LIGHTS)


def regir_cell(P, jitter_draws, centre, cell_size, jitter_scale=JITTER_SCALE):
    """the cell of a surface point: floor((P + j * size - centre) / size) + 8 per axis, j = (r - 0.5) * 2 in float32; -1 outside the grid"""
    P = np.asarray(P, np.float32)
    j = ((np.asarray(jitter_draws, np.float32) - f32(0.5)) * f32(jitter_scale)).astype(np.float32)
    cs = f32(cell_size)
    f = np.floor(((P + (j * cs).astype(np.float32)).astype(np.float32) - np.asarray(centre, np.float32)).astype(np.float32) / cs)
    inside = np.all((f >= -GRID // 2) & (f < GRID // 2), -1)
    i = np.where(inside[..., None], f, 0).astype(np.int64) + GRID // 2
    return np.where(inside, (i[..., 2] * GRID + i[..., 1]) * GRID + i[..., 0], -1)


def screen_tile(x, y, frame, tile_px=SCREEN_TILE):
    """the light tile of global pixel (x, y): seeded by (x / 16, y / 16, FrameIndex)"""
    _, t = rng_next(rng_states(np.asarray(x) // tile_px, np.asarray(y) // tile_px, frame, SALT_SCREEN_TILE))
    return index_of(t, TILE_COUNT)


# ---- initial sampling ----------------------------------------------------------------------------------------------------------------
def candidates(mode, x, y, frame, samples, P, n_lights, tiles_li=None, tiles_inv=None, cells_li=None, cells_w=None, centre=None,
               cell_size=1.0):
    """the candidates of one pixel: list of (light index or -1, source pdf (float32), r1, r2, r3) in draw order"""
    st = rng_states(np.uint64(x), np.uint64(y), frame, R.SALT_INITIAL)
    src = None
    if mode in ("power_ris", "regir"):
        t = int(screen_tile(x, y, frame))
        src = (tiles_li[t * TILE_SIZE:(t + 1) * TILE_SIZE], tiles_inv[t * TILE_SIZE:(t + 1) * TILE_SIZE])
    if mode == "regir":
        j = []
        for _ in range(3):
            st, r = rng_next(st); j.append(r)
        cell = int(regir_cell(P, np.array(j, np.float32), centre, cell_size))
        if cell >= 0:
            src = (cells_li.reshape(-1, CELL_LIGHTS)[cell], cells_w.reshape(-1, CELL_LIGHTS)[cell])
    out = []
    for _ in range(samples):
        d = []
        for _ in range(4):
            st, r = rng_next(st); d.append(r)
        r0, r1, r2, r3 = d
        if src is None:
            li, pdf = int(index_of(r0, n_lights)), f32(1.0) / f32(n_lights)
        else:
            k = int(index_of(r0, len(src[0])))
            li, inv = int(src[0][k]), f32(src[1][k])
            pdf = f32(1.0) / inv if li >= 0 else f32(0)
        out.append((li, pdf, r1, r2, r3))
    return out


def initial_reservoir(S, pix, cands, lights, bsdf, samples):
    """streaming RIS over the candidates of one pixel (float64 p-hat); returns (LightIndex, U, V, W, M, margin)"""
    lis = [c[0] for c in cands]
    margins = []
    p = R.target_pdfs(S, [pix] * len(cands), lights, lis, [c[2] for c in cands], [c[3] for c in cands], bsdf, margins)
    wsum, sel, psel, margin = 0.0, None, 0.0, np.inf
    for k, (li, pdf, r1, r2, r3) in enumerate(cands):
        w = p[k] / float(pdf) if (li >= 0 and p[k] > 0) else 0.0
        wsum += w
        if w > 0:
            margin = min(margin, R._margin(float(r3) * wsum, w), margins[k])
        if float(r3) * wsum < w:
            sel, psel = k, p[k]
    if sel is None or not psel > 0:
        return -1, 0.0, 0.0, 0.0, samples, margin
    c = cands[sel]
    return c[0], float(c[2]), float(c[3]), wsum / samples / psel, samples, margin
