"""The rig, objects and states of the pose-parity checks (tests/test_animation_gpu.py) and of the looseness check of the bound
(tests/test_animation_rules.py): a chain of depth 5 with one branch (7 nodes), 3 clips, two objects sharing the rig.

Node forest (depth first):  0 - 1 - 2 - 3 - 4      Clip 0 (4 s): the slerp cases on node 1 (90 degrees | 179.9 degrees | a negative dot | the lerp branch),
                                \\                              rotations about other axes on nodes 2 and 3, translations on 0 and 4, a scale on 5
                                 5 - 6              Clip 1 (2 s): single-key channels, a channel that starts late (0.25 s)
                                                    Clip 2 (0 s): one key at time 0: Duration 0, posed at time 0 whatever the Time
"""
import math

import numpy as np

import __graft_entry__ as ge

NO_NODE = 0xFFFFFFFF


def quat(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    h = math.radians(deg) / 2
    return tuple(float(np.float32(v)) for v in (a[0] * math.sin(h), a[1] * math.sin(h), a[2] * math.sin(h), math.cos(h)))


def affine(t, axis, deg, s):
    """row-vector S . R . T as float32 [4, 4]"""
    ge.load_package()
    import dxpbrt_amd.ingest as I
    m = np.diag([s[0], s[1], s[2], 1.0]) @ I.matrix_from_quaternion(quat(axis, deg))
    tr = np.eye(4); tr[3, :3] = t
    return (m @ tr).astype(np.float32)


def parity_rig(S):
    Z, X, A = (0, 0, 1), (1, 0, 0), (1, 2, -1)
    ident = (0.0, 0.0, 0.0, 1.0)
    rest = [(0.2, 0.1, -0.3) + quat(Z, 10) + (1.0, 1.25, 0.8), (0.0, 0.5, 0.0) + ident + (1.0, 1.0, 1.0),
            (0.1, 0.4, 0.0) + quat(A, 25) + (0.9, 1.1, 1.0), (0.0, 0.3, 0.1) + quat(X, -15) + (1.0, 1.0, 1.0),
            (0.0, 0.25, 0.0) + ident + (1.2, 0.7, 1.0), (0.4, 0.0, 0.2) + quat(A, -40) + (0.5, 0.5, 0.75), (-0.1, 0.2, 0.3) + quat(Z, 70) + (1.0, 2.0, 1.0)]
    neg = tuple(-v for v in quat(Z, 300.0))                     # the same rotation, the other sign: its dot with the key before it is negative
    clip0 = {(1, 1): ([0.0, 1.0, 2.0, 3.0, 4.0], [quat(Z, 0), quat(Z, 90), quat(Z, 269.9), neg, tuple(-v for v in quat(Z, 300.2))]),
             (2, 1): ([0.0, 1.5, 4.0], [quat(A, 0), quat(A, 120), quat(X, 45)]),
             (3, 1): ([0.5, 3.5], [quat(X, -30), quat((0, 1, 0), 60)]),
             (0, 0): ([0.0, 2.0, 4.0], [(0.2, 0.1, -0.3), (0.5, 0.3, -0.1), (-0.2, 0.0, 0.4)]),
             (4, 0): ([1.0, 3.0], [(0.0, 0.25, 0.0), (0.3, 0.5, -0.2)]),
             (5, 2): ([0.0, 4.0], [(0.5, 0.5, 0.75), (1.5, 0.75, 0.5)])}
    clip1 = {(2, 1): ([1.0], [quat(A, 200)]), (6, 0): ([0.0], [(0.3, -0.2, 0.1)]), (3, 0): ([0.25, 2.0], [(0.0, 0.3, 0.1), (0.2, 0.6, 0.1)]),
             (1, 1): ([0.0, 2.0], [quat(X, 0), quat(X, 150)])}
    clip2 = {(3, 1): ([0.0], [quat(Z, 33)])}
    return S.rig_from_channels([-1, 0, 1, 2, 3, 1, 5], rest, [clip0, clip1, clip2], names=[f"n{i}" for i in range(7)])


def parity_objects(S):
    rig = parity_rig(S)
    ib = lambda k: affine((0.1 * k, -0.2, 0.05 * k), (1, k, 2), 20.0 * k, (1.0, 1.0 + 0.1 * k, 0.9))
    a = S.AnimatedObject(rig, affine((0.5, 0.0, -1.0), (0, 1, 0), 35.0, (1.0, 1.0, 1.0)),
                         np.array([4, NO_NODE, 6], np.uint32), np.array([0, 1, 2], np.uint32),
                         np.stack([np.eye(4, dtype=np.float32), affine((1, 2, 3), (0, 0, 1), 30, (2, 1, 1)), np.eye(4, dtype=np.float32)]),
                         [S.Skin(1, np.array([2, 3, 4, NO_NODE], np.uint32), np.stack([ib(k) for k in range(4)])),
                          S.Skin(NO_NODE, np.array([5], np.uint32), np.stack([ib(5)])),
                          S.Skin(5, np.array([6, 0], np.uint32), np.stack([ib(6), ib(7)]))])
    b = S.AnimatedObject(rig, affine((-1.0, 0.2, 0.0), (1, 0, 0), -20.0, (1.5, 1.5, 1.5)),
                         np.array([3], np.uint32), np.array([3], np.uint32), np.eye(4, dtype=np.float32)[None],
                         [S.Skin(2, np.array([3, 4], np.uint32), np.stack([ib(2), ib(3)]))])
    return [a, b]


# (clip, time) of object A | of object B, posed together in one pt_anim_evaluate. Exactly on keys (1.0, 2.0, 0.5, 3.5), before the first key
# of a channel (0.25 < 0.5, 0.1 < 0.25), at and after the last key (4.0, 5.0), inside each slerp case of clip 0's node 1, the Duration-0 clip.
STATES = [((0, 0.0), (1, 0.1)), ((0, 0.25), (1, 0.25)), ((0, 0.37), (1, 1.0)), ((0, 1.0), (1, 1.3)), ((0, 1.6), (2, 0.0)), ((0, 2.0), (2, 7.5)),
          ((0, 2.45), (0, 3.999)), ((0, 3.3), (0, 0.5)), ((0, 3.5), (1, 2.0)), ((0, 4.0), (1, 5.0)), ((0, 5.0), (0, 3.75)), ((1, 0.7), (0, 1.0))]
