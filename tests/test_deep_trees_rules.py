"""tests/deepsets.py without a GPU: the generators, the depths they are made for, and what the replay of a trace log accepts and notices.

Depths predicted by bvhref.build with the restated parameters (top level / deepest bottom level, 2 (t + b) + 4 as check_depth adds it up):
  deep_small       0 / 19   42   441 triangles, a traversal copy of 38 KB (staged in LDS)
  deep_large       0 / 25   54   4410 triangles: past the single-workgroup collapse
  deep_two_level  13 / 17   64   the deepest structure that is accepted
  too_deep        14 / 17   66   the shallowest that is refused
  deeper_mesh     13 / 19   68   deep_two_level after its bottom level was updated to a deeper mesh: refused
The host walk (deepsets.walk_log: trace_single's loop over a hand-assembled copy, with a model of GroupStack) writes the log the device
writes; replay() must accept it. Then ONE thing is damaged in the model stack at a time -- the faults that can hide where a stack leaves its
LDS part -- and replay() must say so. tests/test_deep_trees_gpu.py asks the same replay of the logs the device writes."""
import numpy as np
import pytest

import bvh_check
import deepsets as D
import isectref as R
import isectsets as I
from test_bvh_builder_rules import full_check, leaf_rule

f32 = np.float32

FLOORS = {"deep_small": (0, 17), "deep_large": (0, 20), "deep_two_level": (8, 17), "too_deep": (8, 17), "deeper_mesh": (8, 17)}
PREDICTED = {"deep_small": (0, 19), "deep_large": (0, 25), "deep_two_level": (13, 17), "too_deep": (14, 17), "deeper_mesh": (13, 19)}


def test_the_generators_are_deterministic():
    a, sa = D.nested_shells(30, 16)
    b, sb = D.nested_shells(30, 16)
    assert a.dtype == f32 and a.shape == (480, 3, 3) and a.tobytes() == b.tobytes() and np.array_equal(sa, sb)
    assert a.tobytes() != D.nested_shells(30, 16, seed=1)[0].tobytes()
    cells, rest = D.shell_cells(30)
    for k, (lo, hi) in enumerate(cells):                                       # every triangle inside its own half-cell
        t = a[sa == k].astype(np.float64)
        assert (t >= lo).all() and (t <= hi).all(), k
    assert np.array_equal(rest[1], [2.0 ** -10] * 3)
    xa, xb = D.nested_instances(24, 8)[0], D.nested_instances(24, 8)[0]
    assert len(xa) == 192 and all(p.tobytes() == q.tobytes() for p, q in zip(xa, xb))
    for name in ("deep_small", "deep_two_level"):
        r0, k0, _ = D.deep_rays(name)
        r1, k1, _ = D.deep_rays.__wrapped__(name)
        assert r0.shape == (D.RAYS, 8) and r0.tobytes() == r1.tobytes() and np.array_equal(k0, k1)
        d = r0[:, 4:7]
        assert ((d == 0) | (np.abs(d) == f32(1e-30))).any(1).sum() >= D.RAYS // 16 - 1      # zero, -0.0 and +-1e-30 components
        assert np.isfinite(r0[:, 7]).sum() == D.RAYS // 10 and sorted(set(k0.tolist())) == [0, 1, 2, 3]
        assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()


@pytest.mark.parametrize("name", list(D.SPECS))
def test_predicted_depths(name):
    t, b = D.predicted_depths(name)
    meshes, objects = D.geometry(name)
    print(f"[deep] {name}: top level {t}, bottom level {b}, 2 (t + b) + 4 = {D.stack_budget(name)}, {sum(len(m) for m in meshes)} triangles, {len(objects)} instances")
    assert t >= FLOORS[name][0] and b >= FLOORS[name][1]
    assert (t, b) == PREDICTED[name], "the docstrings and DESIGN.md quote these"
    if name == "deep_small":
        lay, buf, _ = D.assembled(name)
        # the device's copy holds one entry record (144 B) more than the assembled one, and as many top-level nodes
        assert len(objects) == 1 and len(buf) + 144 <= D.BLOB_LDS_MAX, "the traversal copy must fit the LDS staging"
    if name == "deep_large":
        assert len(meshes[0]) > D.SINGLE_GROUP_LEAVES and len(meshes[0]) * 64 > D.BLOB_LDS_MAX       # one triangle per leaf
    if name == "deep_two_level":
        assert D.stack_budget(name) in (62, 64) and D.stack_budget(name) <= D.STACK_SIZE
        assert objects[-1][0] == 1 and len(objects) == 45 * 6 + 1
    if name in ("too_deep", "deeper_mesh"):
        assert D.stack_budget(name) >= 66


def test_the_assembled_deep_small_passes_both_checkers():
    lay, buf, trees = D.assembled("deep_small")
    stats = bvh_check.check_blob(lay, buf, leaf_rule)
    res = full_check(lay, buf)
    (T, r, _), = res["trees"].values()
    assert stats["blas_depth"] == r["depth"] == D.predicted_depths("deep_small")[1]
    assert r["cost"] <= r["optimum"] * (1 + 1e-12)


# ---------------------------------------------------------------------------------------------
# the records the device is held to: the oracle's brute force, against its own tree and against the exact closest hit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep_small", "deep_large", "deep_two_level"])
def test_oracle_records_of_the_deep_rays(oracle, name):
    """tests/test_deep_trees_gpu.py demands the device's records to equal the oracle's brute force bit for bit; here those records are
    checked: the oracle's own tree finds the same, and a sample of 200 is the exact closest hit within isectref's bounds"""
    soup, rays = D.scene(name)
    brute = I.oracle_closest(oracle, soup.scene, rays, accel_mode=0)
    assert not I.same_records(I.oracle_closest(oracle, soup.scene, rays, accel_mode=1), brute), name
    hit = brute["Instance"] != I.MISS
    kind = D.deep_rays(name)[1]
    assert hit.mean() > 0.1 and all(hit[kind == k].any() for k in range(4)), "every kind of ray must hit something somewhere"
    sel = np.arange(0, len(rays), len(rays) // 200)[:200]
    fig = R.check_closest(rays[sel], soup.instances, brute[sel], soup.slot_of, f"oracle, {name}")
    print(f"[deep] {name}: {hit.mean():.1%} of {len(rays)} rays hit; exact closest on {len(sel)}: {fig}")


# ---------------------------------------------------------------------------------------------
# the replay accepts the host walk, and the walk goes where the GPU tests need it
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walks():
    out = {}
    for name in ("deep_small", "deep_two_level"):
        lay, buf, _ = D.assembled(name)
        rays = D.deep_rays(name)[0]
        out[name] = (lay, buf, [(i, D.walk_log(lay, buf, rays[i])) for i in D.logged_rays(name)])
    return out


@pytest.mark.parametrize("name", ["deep_small", "deep_two_level"])
def test_replay_accepts_the_host_walk(walks, name):
    lay, buf, logs = walks[name]
    assert len(logs) == D.LOGGED
    res = [D.replay(log, lay.InstanceCount == 1) for _, log in logs]
    sp = np.array([r["max_sp"] for r in res]); lv = np.array([r["blas_levels"] for r in res])
    print(f"[deep] {name}: host walk, max sp {sp.max()} (>= 16 on {(sp >= 16).sum()}, >= 24 on {(sp >= 24).sum()} of {len(sp)}), "
          f"levels owed inside the bottom level {lv.max()} (>= 12 on {(lv >= 12).sum()}), longest log {max(r['steps'] for r in res)} steps")
    assert (sp >= 16).sum() >= 32 and (lv >= D.STACK_LDS_PHASED + 4).sum() >= 32
    assert all(int(log[:, 3].max()) == r["max_sp"] for (_, log), r in zip(logs, res))
    if name == "deep_two_level":
        assert (sp >= 24).any()
        # the parked top-level state straddles the LDS boundary on some ray: sp at an entry (code 1) in 10 .. 11
        assert any(((log[:, 0] == 1) & (log[:, 3] > D.LDS_DEPTH - 3) & (log[:, 3] < D.LDS_DEPTH)).any() for _, log in logs)


def deepest(walks, name):
    lay, buf, logs = walks[name]
    i, log = max(logs, key=lambda il: int(il[1][:, 3].max()))
    return lay, buf, D.deep_rays(name)[0][i]


@pytest.mark.parametrize("fault", ["neighbour", "deeper", "shallower", "handover"])
@pytest.mark.parametrize("name", ["deep_small", "deep_two_level"])
def test_replay_notices_a_damaged_private_part(walks, name, fault):
    """neighbour: a pop returns a neighbour's entry; deeper / shallower: the entry of depth + 1 / - 1 (the index sp - LDS_DEPTH off by
    one); handover: push and pop disagree about where entry LDS_DEPTH lives (sp <= LDS_DEPTH in one of them)"""
    lay, buf, ray = deepest(walks, name)
    one = lay.InstanceCount == 1
    sound = D.ModelStack()
    D.replay(D.walk_log(lay, buf, ray, sound), one)
    assert sound.fired == 0
    stack = D.ModelStack(fault=fault)
    log = D.walk_log(lay, buf, ray, stack)
    assert stack.fired > 0, "the ray never pops from the private part"
    with pytest.raises(AssertionError, match="the pop returns|the model stack holds|restored|cut short|no end|not the current one"):
        D.replay(log, one)


@pytest.mark.parametrize("lds_depth", [2, 3])
def test_replay_notices_parked_state_lost_at_the_boundary(walks, lds_depth):
    """the entries of an instance transition with the hand-over among them: a stack whose LDS part ends at the marker (2) or just above
    it (3: the first node group of the bottom level) loses that entry. (The T parked under the marker of a one-instance scene is
    (0, 0), which is also what a lost entry reads as: the two-level scene of test_replay_notices_a_damaged_private_part covers T.)"""
    lay, buf, ray = deepest(walks, "deep_small")
    D.replay(D.walk_log(lay, buf, ray, D.ModelStack(lds_depth=lds_depth)), True)          # a sound stack of that split is fine
    stack = D.ModelStack(lds_depth=lds_depth, fault="handover")
    log = D.walk_log(lay, buf, ray, stack)
    assert stack.fired > 0
    with pytest.raises(AssertionError):
        D.replay(log, True)


def test_replay_notices_a_damaged_log(walks):
    """the log itself: a wrong sp, a restored state that is not the parked one, a missing end, a result after the end"""
    lay, buf, ray = deepest(walks, "deep_two_level")
    log = D.walk_log(lay, buf, ray)
    D.replay(log, False)
    k6 = int(np.nonzero(log[:, 0] == 6)[0][0]); k5 = int(np.nonzero((log[:, 0] == 5) & (log[:, 3] >= D.LDS_DEPTH))[0][0])
    for row, col, delta, what in ((k5, 3, 1, "the model stack holds"), (k5, 1, 1, "the pop returns"), (k6, 2, 1, "restored"), (k6, 1, 0x100, "restored")):
        bad = log.copy(); bad[row, col] += delta
        with pytest.raises(AssertionError, match=what):
            D.replay(bad, False)
    with pytest.raises(AssertionError, match="no end"):
        D.replay(log[:-1], False)
    with pytest.raises(AssertionError, match="cut short"):
        D.replay(np.concatenate([log[:-1], np.zeros((1, 4), np.uint32)]), False)
    with pytest.raises(AssertionError, match="after its end"):
        D.replay(np.concatenate([log, log[-1:]]), False)
