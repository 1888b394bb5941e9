"""Float64 restatement of the animation pose ("Animation"; Source/Animation.ixx:45-75, 119-162; Source/Scene.ixx:195-231),
with a first-order running error bound for the device's fp32 evaluation next to every number it returns.

Independent of the device code: numpy only, written from Animation.ixx and the spec. Every quantity is a `Bd`: a float64 value and a bound on
|fp32 result - value|, carried through the operations in the device's stated order:
    a + b, a - b   e = ea + eb + u |a + b|
    a * b          e = |a| eb + |b| ea + u |a b|
    a / b          e = ea / |b| + |a / b| eb / |b| + u |a / b|
    f(a)           e = |f'(a)| ea + K u |f(a)|           (sqrtf, atan2f, sinf; K below)
with u = 2^-24 per rounding. Through a matrix product this is |EA||B| + |A||EB| + gamma |A||B| entry by entry (gamma from the three sums and
the product of the stated order); through the cofactor inverse the propagated part is, to first order, |M^-1||dM||M^-1|, and the rest is the
rounding of the cofactor arithmetic itself. Second-order terms are neglected: with cond(Global(meshNode)) <= 1e3 (the fixtures keep it; the
tests assert it) they stay below 1e-4 of the bound, and tests compare against 2 x bound.

The device's sqrtf / atan2f / sinf errors cannot be derived from the number format. tests/test_animation_gpu.py measures them against float64
on the slerp cases of its own pose set (pt_anim_debug_slerp hands out the intermediates) and asserts measured <= K / 2:
    measured on gfx950 (ROCm 7.2 device library), relative error in units of u:  sqrtf 0.850   atan2f 1.606   sinf 1.003
K is twice the measured maximum, rounded up in the last digit.
"""
import numpy as np

U = 2.0 ** -24
K_SQRT, K_ATAN2, K_SIN = 1.71, 3.22, 2.01
MEASURED = {"sqrtf": 0.850, "atan2f": 1.606, "sinf": 1.003}      # what the constants above are twice of
NO_NODE = 0xFFFFFFFF
MUTANTS = ("order", "one_minus_t", "sign_flip", "transposed")


class Bd:
    """values (float64, any shape) with a first-order bound on the fp32 evaluation's absolute error"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, Bd) else Bd(x)

    def __getitem__(self, k):
        return Bd(self.v[k], self.e[k])

    def __neg__(self):
        return Bd(-self.v, self.e)

    def __add__(self, o):
        o = Bd.of(o); v = self.v + o.v
        return Bd(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        o = Bd.of(o); v = self.v - o.v
        return Bd(v, self.e + o.e + U * np.abs(v))

    def __mul__(self, o):
        o = Bd.of(o); v = self.v * o.v
        return Bd(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(v))

    def __truediv__(self, o):
        o = Bd.of(o); v = self.v / o.v
        return Bd(v, self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v) + U * np.abs(v))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return Bd.of(o) - self

    @property
    def T(self):
        return Bd(self.v.T, self.e.T)


def stack(rows):
    """a Bd matrix from nested lists of Bd / float scalars"""
    rows = [[Bd.of(x) for x in r] for r in rows]
    return Bd(np.array([[float(x.v) for x in r] for r in rows]), np.array([[float(x.e) for x in r] for r in rows]))


def exact_negate_column(m, col):
    v, e = m.v.copy(), m.e.copy()
    v[:, col] = -v[:, col]
    return Bd(v, e)


# ---- the arithmetic of the spec -----------------------------------------------------------------------------------------------------------
def matmul(a, b):
    """C = A . B, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3"""
    p = [a[:, k:k + 1] * b[k:k + 1, :] for k in range(4)]
    return ((p[0] + p[1]) + p[2]) + p[3]


def inverse(m):
    """the general 4x4 cofactor inverse, the device's order"""
    g = lambda i: m[i // 4, i % 4]
    s0 = g(0) * g(5) - g(4) * g(1); s1 = g(0) * g(6) - g(4) * g(2); s2 = g(0) * g(7) - g(4) * g(3)
    s3 = g(1) * g(6) - g(5) * g(2); s4 = g(1) * g(7) - g(5) * g(3); s5 = g(2) * g(7) - g(6) * g(3)
    c5 = g(10) * g(15) - g(14) * g(11); c4 = g(9) * g(15) - g(13) * g(11); c3 = g(9) * g(14) - g(13) * g(10)
    c2 = g(8) * g(15) - g(12) * g(11); c1 = g(8) * g(14) - g(12) * g(10); c0 = g(8) * g(13) - g(12) * g(9)
    det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0
    r = Bd(1.0) / det
    o = [None] * 16
    o[0] = ((g(5) * c5 - g(6) * c4) + g(7) * c3) * r
    o[1] = ((-g(1) * c5 + g(2) * c4) - g(3) * c3) * r
    o[2] = ((g(13) * s5 - g(14) * s4) + g(15) * s3) * r
    o[3] = ((-g(9) * s5 + g(10) * s4) - g(11) * s3) * r
    o[4] = ((-g(4) * c5 + g(6) * c2) - g(7) * c1) * r
    o[5] = ((g(0) * c5 - g(2) * c2) + g(3) * c1) * r
    o[6] = ((-g(12) * s5 + g(14) * s2) - g(15) * s1) * r
    o[7] = ((g(8) * s5 - g(10) * s2) + g(11) * s1) * r
    o[8] = ((g(4) * c4 - g(5) * c2) + g(7) * c0) * r
    o[9] = ((-g(0) * c4 + g(1) * c2) - g(3) * c0) * r
    o[10] = ((g(12) * s4 - g(13) * s2) + g(15) * s0) * r
    o[11] = ((-g(8) * s4 + g(9) * s2) - g(11) * s0) * r
    o[12] = ((-g(4) * c3 + g(5) * c1) - g(6) * c0) * r
    o[13] = ((g(0) * c3 - g(1) * c1) + g(2) * c0) * r
    o[14] = ((-g(12) * s3 + g(13) * s1) - g(14) * s0) * r
    o[15] = ((g(8) * s3 - g(9) * s1) + g(10) * s0) * r
    return stack([o[0:4], o[4:8], o[8:12], o[12:16]])


def slerp(q0, q1, t, mutant=None):
    """XMQuaternionSlerp's structure on Bd quaternions (x, y, z, w); not renormalised. Returns (q, branch): branch 'lerp' or 'slerp'."""
    q0, q1, t = Bd.of(q0), Bd.of(q1), Bd.of(t)
    c = ((q0[0] * q1[0] + q0[1] * q1[1]) + q0[2] * q1[2]) + q0[3] * q1[3]
    if float(c.v) < 0.0:
        c = -c
        if mutant != "sign_flip":
            q1 = -q1
    if float(c.v) > 1.0 - 1e-5:
        w0, w1, branch = Bd(1.0) - t, t, "lerp"
    else:
        x = Bd(1.0) - c * c
        s = Bd(np.sqrt(x.v), x.e / (2.0 * np.sqrt(x.v)) + K_SQRT * U * np.sqrt(x.v))
        w = np.arctan2(s.v, c.v)
        w = Bd(w, (np.abs(c.v) * s.e + np.abs(s.v) * c.e) / (s.v * s.v + c.v * c.v) + K_ATAN2 * U * np.abs(w))
        a0, a1 = (Bd(1.0) - t) * w, t * w
        sin = lambda a: Bd(np.sin(a.v), np.abs(np.cos(a.v)) * a.e + K_SIN * U * np.abs(np.sin(a.v)))
        w0, w1, branch = sin(a0) / s, sin(a1) / s, "slerp"
    if mutant == "one_minus_t":
        w0, w1 = w1, w0
    return w0 * q0 + w1 * q1, branch


def find_key(times, time):
    """KeyframeCollection::FindKey: upper_bound - 1, or len(times) past the last key"""
    k = int(np.searchsorted(np.asarray(times, np.float64), time, side="right"))
    return len(times) if k == len(times) else k - 1


def interpolate(times, values, time, rotation, mutant=None):
    """KeyframeCollection::Interpolate without the matrix: the channel's value at `time` (Bd, 3 or 4 components)"""
    times = np.asarray(times, np.float64); values = np.asarray(values, np.float64)
    n = 4 if rotation else 3
    if time < times[0]:
        return Bd(values[0][:n])
    i = find_key(times, time)
    if i == len(times):
        return Bd(values[-1][:n])
    t = (time - times[i]) / (times[i + 1] - times[i])
    t = Bd(t, U * abs(t))                                   # rounded to fp32 once (the fp64 quotient's own error is 2^-29 of that)
    a, b = Bd(values[i][:n]), Bd(values[i + 1][:n])
    if rotation:
        return slerp(a, b, t, mutant)[0]
    if mutant == "one_minus_t":
        a, b = b, a
    return a + t * (b - a)


def local_matrix(tr, q, sc, mutant=None):
    """S . R . T with XMMatrixRotationQuaternion's R; the products with the zeros and ones of S and T are exact"""
    tr, q, sc = Bd.of(tr), Bd.of(q), Bd.of(sc)
    x, y, z, w = q[0], q[1], q[2], q[3]
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz, xw, yw, zw = x * y, x * z, y * z, x * w, y * w, z * w
    two, one = Bd(2.0), Bd(1.0)
    r = [[one - two * (yy + zz), two * (xy + zw), two * (xz - yw)],
         [two * (xy - zw), one - two * (xx + zz), two * (yz + xw)],
         [two * (xz + yw), two * (yz - xw), one - two * (xx + yy)]]
    if mutant == "order":                                   # T . R . S in place of S . R . T
        rm = stack([r[0] + [0.0], r[1] + [0.0], r[2] + [0.0], [0.0, 0.0, 0.0, 1.0]])
        tm = stack([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [tr[0], tr[1], tr[2], 1.0]])
        sm = stack([[sc[0], 0, 0, 0], [0, sc[1], 0, 0], [0, 0, sc[2], 0], [0, 0, 0, 1.0]])
        return matmul(matmul(tm, rm), sm)
    rows = [[sc[i] * r[i][j] for j in range(3)] + [0.0] for i in range(3)]
    return stack(rows + [[tr[0], tr[1], tr[2], 1.0]])


# ---- the pose -----------------------------------------------------------------------------------------------------------------------------
def pose(rig, clip, time, mutant=None):
    """Animation::ComputeTransforms: the global transform of every node of `rig` (scenes.Rig) at `time` of `clip`: a list of Bd 4x4."""
    if float(rig.durations[clip]) == 0.0:
        time = 0.0
    out = []
    for n in range(len(rig.parents)):
        rest = np.asarray(rig.rest[n], np.float64)
        val = [Bd(rest[0:3]), Bd(rest[3:7]), Bd(rest[7:10])]
        for path in range(3):
            first, count = (int(v) for v in rig.channels[clip, n, path])
            if count:
                val[path] = interpolate(rig.key_times[first:first + count], rig.key_values[first:first + count], time, path == 1, mutant)
        m = local_matrix(val[0], val[1], val[2], mutant)
        p = int(rig.parents[n])
        out.append(m if p < 0 else matmul(m, out[p]))
    return out


def store3x4(m, mutant=None):
    """XMStoreFloat3x4: the first three rows of the transpose"""
    return m[:3, :] if mutant == "transposed" else m.T[:3, :]


def skeletal_transforms(obj, globals_, skin, mutant=None):
    """(InverseBind . Global(joint)) . Global(meshNode)^-1 per joint of obj.skins[skin] as float3x4: a list of Bd [3, 4], None for a matrix
    the device leaves as it was (no node for the joint or the mesh node)."""
    s = obj.skins[skin]
    if int(s.mesh_node) == NO_NODE:
        return [None] * len(s.joint_nodes)
    inv = inverse(globals_[int(s.mesh_node)])
    out = []
    for j, jn in enumerate(s.joint_nodes):
        if int(jn) == NO_NODE:
            out.append(None)
            continue
        out.append(store3x4(matmul(matmul(Bd(np.asarray(s.inverse_binds[j], np.float64)), globals_[int(jn)]), inv), mutant))
    return out


def instance_transforms(obj, globals_, mutant=None):
    """Scene::Refresh: To3x4((Global(meshNode) . Scale(1, 1, -1)) . RenderObject.Transform) per binding: a list of Bd [3, 4]"""
    out = []
    for b, node in enumerate(obj.binding_nodes):
        g = Bd(np.asarray(obj.binding_globals[b], np.float64)) if int(node) == NO_NODE else globals_[int(node)]
        out.append(store3x4(matmul(exact_negate_column(g, 2), Bd(np.asarray(obj.transform, np.float64))), mutant))
    return out


def condition(m):
    return float(np.linalg.cond(np.asarray(m, np.float64)))
