"""Restatement of the ReGIR Onion layout (pt_di_set_regir_layout; DESIGN.md section 1, "Local-light sampling"): the static tables in
float64 (layer boundaries, ring and azimuth thresholds, cell spheres), and, in the device's float32 steps, the lookup of a point's cell,
the distance-scaled jitter, the cell spheres at a scale and the build of a cell's slots. The device rules take the tables as float32
arrays (`Tables`): the tests hand them the library's own (ptamd.onion_table), once those are shown to lie within one float32 ulp of
tables64(), so a last-bit difference between two cos implementations cannot fail a pin. Builds on presamplingref."""
import numpy as np

import presamplingref as P
import restirref as R

f32 = np.float32
PARTITIONS = (8, 12, 16, 20, 24)                    # per layer group
GROUP_LAYERS = (1, 1, 1, 1, 11)
RING_CELLS = ((8, 5, 1), (12, 10, 6, 1), (16, 14, 11, 6, 1), (20, 19, 16, 11, 6, 1), (24, 23, 20, 16, 12, 6, 1))
LAYERS, CELLS = 15, 2253
LAYER_GROUP = tuple(g for g, n in enumerate(GROUP_LAYERS) for _ in range(n))
LAYER_CELLS = tuple(RING_CELLS[g][0] + 2 * sum(RING_CELLS[g][1:]) for g in LAYER_GROUP)
LAYER_BASE = tuple(1 + sum(LAYER_CELLS[:l]) for l in range(LAYERS))
JITTER_PER_DISTANCE = f32(0.2617994)                # pi / 12: one outermost-group cell width per unit distance
ROWS = [(g, k) for g in range(5) for k in range(len(RING_CELLS[g]))]                  # (group, ring) in table order


def diamond64(x, z):
    if abs(x) + abs(z) == 0:
        return 0.0
    if z >= 0:
        return z / (x + z) if x >= 0 else 1 + (-x) / (z - x)
    return 2 + (-z) / (-x - z) if x < 0 else 3 + x / (x - z)


def tables64():
    """(b2 [16], ring thresholds [20], azimuth thresholds [241], cells [2253, 4]) in float64, from the spec"""
    ratio = [(p + np.pi) / (p - np.pi) for p in PARTITIONS]
    B = [1.0]
    for l in range(LAYERS):
        B.append(B[-1] * ratio[LAYER_GROUP[l]])
    ring = [np.sin((k - 0.5) * 2 * np.pi / p) ** 2 for p in PARTITIONS for k in range(1, p // 4 + 1)]
    az = [diamond64(np.cos(2 * np.pi * j / n), np.sin(2 * np.pi * j / n)) for g, k in ROWS for n in [RING_CELLS[g][k]] for j in range(1, n)]

    def point(r, E, A):
        return np.array([r * np.cos(E) * np.cos(A), r * np.sin(E), r * np.cos(E) * np.sin(A)])

    cells = [(0.0, 0.0, 0.0, 1.0)]
    for l in range(LAYERS):
        g = LAYER_GROUP[l]
        p = PARTITIONS[g]
        eq = 2 * np.pi / p
        r_in, r_out = B[l], B[l + 1]
        r_mid = 0.5 * (r_in + r_out)
        for k, n in enumerate(RING_CELLS[g]):
            lo, hi = (k - 0.5) * eq, (np.pi / 2 if k == p // 4 else (k + 0.5) * eq)
            for sgn in ((1.0,) if k == 0 else (1.0, -1.0)):
                for i in range(n):
                    if n == 1:
                        c = np.array([0.0, sgn * r_mid, 0.0])
                        corners = [point(r, sgn * lo, 0.0) for r in (r_in, r_out)]
                        rad = max([r_out - r_mid] + [np.linalg.norm(c - q) for q in corners])
                    else:
                        c = point(r_mid, sgn * k * eq, (i + 0.5) * 2 * np.pi / n)
                        corners = [point(r, sgn * E, A) for r in (r_in, r_out) for E in (lo, hi) for A in (i * 2 * np.pi / n, (i + 1) * 2 * np.pi / n)]
                        rad = max(np.linalg.norm(c - q) for q in corners)
                    cells.append((c[0], c[1], c[2], rad))
    return np.array(B) ** 2, np.array(ring), np.array(az), np.array(cells)


class Tables:
    """the float32 tables the device rules read, with the static row structure"""

    def __init__(self, b2, ring, azimuth, cells):
        self.b2, self.ring, self.azimuth = (np.asarray(a, f32).reshape(-1) for a in (b2, ring, azimuth))
        self.cells = np.asarray(cells, f32).reshape(-1, 4)
        assert (len(self.b2), len(self.ring), len(self.azimuth), len(self.cells)) == (16, 20, 241, CELLS)
        self.ring_of_group, self.az_of_row, self.cell_of_row = [], {}, {}
        at = az = 0
        for g, p in enumerate(PARTITIONS):
            self.ring_of_group.append(self.ring[at:at + p // 4]); at += p // 4
            off = 0
            for k, n in enumerate(RING_CELLS[g]):
                self.az_of_row[g, k] = self.azimuth[az:az + n - 1]; az += n - 1
                self.cell_of_row[g, k] = off                       # ring k north within its layer
                off += n if k == 0 else 2 * n


def diamond32(x, z):
    """the monotone pseudo-angle of (x, z) in [0, 4), float32, the device's branches"""
    x, z = np.asarray(x, f32), np.asarray(z, f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q0 = np.where((x + z).astype(f32) > 0, z / (x + z).astype(f32), f32(0))
        q1 = f32(1) + ((-x) / (z - x).astype(f32)).astype(f32)
        q2 = f32(2) + ((-z) / (-x - z).astype(f32)).astype(f32)
        q3 = f32(3) + (x / (x - z).astype(f32)).astype(f32)
    return np.where(z >= 0, np.where(x >= 0, q0, q1), np.where(x < 0, q2, q3)).astype(f32)


def _rel(v, t):
    """relative distance of v to the nearest of the thresholds t (t > 0)"""
    t = np.asarray(t, np.float64)
    return np.min(np.abs(np.float64(v) - t) / t) if len(t) else np.inf


def lookup(T, v, c, south_first=False, azimuth_from_zero=False, margins=None):
    """the cell of each vector v [.., 3] (relative to the centre) at scale c; -1: no cell. margins (a list): gets, per vector, the smallest
    relative distance of a compared value to a threshold it was compared with (and of the azimuth to its wrap at 0 / 4). south_first,
    azimuth_from_zero: mutations."""
    v = np.asarray(v, f32).reshape(-1, 3)
    if len(v) == 1:                                  # presamplingref._fma keeps arrays of two and more
        return lookup(T, np.repeat(v, 2, 0), c, south_first, azimuth_from_zero, [] if margins is None else margins)[:1]
    c = f32(c)
    d2 = P._dot32(v, v)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (d2 / f32(c * c)).astype(f32)
        e = ((v[:, 1] * v[:, 1]).astype(f32) / d2).astype(f32)
    A = diamond32(v[:, 0], v[:, 2])
    out = np.full(len(v), -1, np.int64)
    for i in range(len(v)):
        m = _rel(q[i], T.b2) if np.isfinite(q[i]) else np.inf
        if not q[i] < T.b2[15]:
            cell = -1
        elif q[i] < f32(1):
            cell = 0
        else:
            layer = int((T.b2[1:15] <= q[i]).sum())
            g = LAYER_GROUP[layer]
            ring = int((T.ring_of_group[g] <= e[i]).sum())
            n = RING_CELLS[g][ring]
            az = T.az_of_row[g, ring]
            k = int((az <= A[i]).sum()) + (1 if azimuth_from_zero else 0)
            south = ring >= 1 and v[i, 1] < 0
            cell = LAYER_BASE[layer] + T.cell_of_row[g, ring] + (n if south != (south_first and ring >= 1) else 0) + k
            m = min(m, _rel(e[i], T.ring_of_group[g]), _rel(A[i], az))
            if n > 1:
                m = min(m, float(A[i]) / 4.0, (4.0 - float(A[i])) / 4.0)
        out[i] = cell
        if margins is not None:
            margins.append(m)
    return out


def jittered(Pw, jitter_draws, centre, cell_size, half=True, distance_term=True):
    """(v, c): the looked-up vector of surface point Pw [.., 3] with the three draws [.., 3], and the scale. half=False (c = the cell
    size), distance_term=False (the jitter scale is c): mutations."""
    c = f32(0.5) * f32(cell_size) if half else f32(cell_size)
    j = ((np.asarray(jitter_draws, f32) - f32(0.5)) * f32(P.JITTER_SCALE)).astype(f32)
    v0 = (np.asarray(Pw, f32) - np.asarray(centre, f32)).astype(f32)
    s = np.maximum(c, (JITTER_PER_DISTANCE * np.sqrt(P._dot32(v0, v0)).astype(f32)).astype(f32)) if distance_term else c
    s = np.asarray(s, f32)
    return (v0 + (j * s[..., None]).astype(f32)).astype(f32), c


def onion_cell(T, Pw, jitter_draws, centre, cell_size, margins=None, **mutations):
    v, c = jittered(Pw, jitter_draws, centre, cell_size, **{k: mutations.pop(k) for k in ("half", "distance_term") if k in mutations})
    return lookup(T, v, c, margins=margins, **mutations)


def cell_spheres(T, cells, centre, cell_size):
    """float32 (centres [n, 3], radii [n]) of the cells around centre: centre + c * table.xyz (product, then add), c * table.w"""
    c = f32(0.5) * f32(cell_size)
    t = T.cells[np.asarray(cells, np.int64)]
    return (np.asarray(centre, f32) + (c * t[:, :3]).astype(f32)).astype(f32), (c * t[:, 3]).astype(f32)


def onion_build(T, lights, tiles_li, tiles_inv, cells, centre, cell_size, build_samples, frame):
    """k_di_regir_build_onion for every slot of the given cells: (LightIndex int64 [len(cells), 512], weight float32); -1 / 0 = empty.
    presamplingref.regir_build's steps (the same seeds, candidates and weight) against the Onion cells' spheres."""
    cells = np.asarray(cells, np.int64)
    NL = P.CELL_LIGHTS
    g = (cells[:, None] * NL + np.arange(NL)[None, :]).reshape(-1).astype(np.uint64)
    cc, rr = cell_spheres(T, cells, centre, cell_size)
    c, radius = np.repeat(cc, NL, 0), np.repeat(rr, NL)
    rng = P.rng_states(g & np.uint64(0xFFF), g >> np.uint64(12), frame, P.SALT_REGIR)
    _, ct = P.rng_next(P.rng_states(g >> np.uint64(8), np.zeros_like(g), frame, P.SALT_REGIR_COHERENT))
    tile = P.index_of(ct, P.TILE_COUNT)
    wsum = np.zeros(len(g), f32); psel = np.zeros(len(g), f32); sel = np.full(len(g), -1, np.int64)
    for _ in range(build_samples):
        rng, u = P.rng_next(rng)
        rng, r = P.rng_next(rng)
        e = tile * P.TILE_SIZE + P.index_of(u, P.TILE_SIZE)
        li, inv = tiles_li[e], tiles_inv[e].astype(f32)
        ok = li >= 0
        p = np.where(ok, P.volume_weight32(lights, np.where(ok, li, 0), c, radius), f32(0)).astype(f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(p > 0, (p / (f32(1.0) / inv).astype(f32)).astype(f32), f32(0)).astype(f32)
        wsum = (wsum + w).astype(f32)
        take = (r * wsum).astype(f32) < w
        sel = np.where(take, li, sel); psel = np.where(take, p, psel)
    with np.errstate(divide="ignore", invalid="ignore"):
        wt = np.where(psel > 0, (wsum / (psel * f32(build_samples)).astype(f32)).astype(f32), f32(0)).astype(f32)
    return np.where(psel > 0, sel, -1).reshape(len(cells), NL), wt.reshape(len(cells), NL)


def pixel_jitter(x, y, frame):
    """(stream state after them, the three jitter draws) of pixel (x, y): the first draws of the pixel's initial-sampling stream"""
    st = P.rng_states(np.uint64(x), np.uint64(y), frame, R.SALT_INITIAL)
    j = []
    for _ in range(3):
        st, r = P.rng_next(st); j.append(r)
    return st, np.array(j, f32)


def candidates(T, x, y, frame, samples, Pw, tiles_li, tiles_inv, cells_li, cells_w, centre, cell_size, margins=None):
    """the candidates of one pixel in ReGIR mode under the Onion layout, as presamplingref.candidates lists them; also the cell (-1: the
    pixel's Power_RIS tile)"""
    t = int(P.screen_tile(x, y, frame))
    src = (tiles_li[t * P.TILE_SIZE:(t + 1) * P.TILE_SIZE], tiles_inv[t * P.TILE_SIZE:(t + 1) * P.TILE_SIZE])
    st, j = pixel_jitter(x, y, frame)
    cell = int(onion_cell(T, Pw, j, centre, cell_size, margins=margins)[0])
    if cell >= 0:
        src = (cells_li.reshape(-1, P.CELL_LIGHTS)[cell], cells_w.reshape(-1, P.CELL_LIGHTS)[cell])
    out = []
    for _ in range(samples):
        d = []
        for _ in range(4):
            st, r = P.rng_next(st); d.append(r)
        k = int(P.index_of(d[0], len(src[0])))
        li, inv = int(src[0][k]), f32(src[1][k])
        out.append((li, f32(1.0) / inv if li >= 0 else f32(0), d[1], d[2], d[3]))
    return out, cell
