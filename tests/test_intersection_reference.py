"""Which triangle a ray hits, and where, against exact geometry (tests/isectref.py) instead of against the same fp32 recipe written twice.

Every input set of tests/isectsets.py goes through the CPU oracle (or_ray_triangle per pair, or_trace_closest per scene) here, and under
`-m gpu` through pt_debug_trace_closest with and without PT_DEBUG_BRUTE_FORCE: the device's records must equal the oracle's brute-force
records bit for bit (T, U, V included; Slot is the device's packet order and is compared between the two device runs), so what the
exact reference says about the oracle's answers it says about the kernels'.

  random pairs     classification = the exact one wherever every margin is decided, u, v, t within the derived bounds (isectref docstring);
                   the undecided share of the REFERENCE is capped at 1 % before anything is asserted about a rule
  dominant axes    every axis and sign, the ties, exact rays through vertices and edges (the fallback): the kernel's rule without the
                   paper's kx/ky swap against the same rule with it (hit, t and non-zero u, v bit for bit; a zero u or v up to its sign)
  exact zeros      integer origins to interior vertices of an integer-lattice mesh, from both sides: at least one incident triangle is hit
                   and all that are hit report the same T; rays to quarter points of edges: hit, T within the t bound (see
                   test_exact_zeros for why not the same T); rays IN the plane: det = 0 exactly, nothing may be hit
  closed meshes    rays from inside, aimed at vertices and edge points, hostile scales: zero leaks, and the any-hit walk says occluded
  closest of many  the chosen triangle is inside or undecided, nothing inside by margin is closer by more than the t bounds; among
                   bit-identical triangles the lowest (instance, geometry, primitive) wins
  interval rule    tmin / tmax at, one ulp below and one ulp above the reported T: (tmin, tmax) is exclusive at both ends
  launch shape     1, 63, 64, 65, 257 and 20 001 rays give the records of the big batch

test_wrong_rule_breaks_its_assertion is the self-test: each wrong variant of isectref.woop_fp32 / woop_closest, playing the kernel on
these same inputs, must fail the assertion named for it in WRONG_RULE_BREAKS."""
import functools

import numpy as np
import pytest

import isectref as R
import isectsets as I

f32 = np.float32
u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)
UNDECIDED_CAP = 0.01
FIGURES = {}                                                    # what the runs measured, printed by the last test of each side


def note(side, name, fig):
    FIGURES.setdefault(side, {})[name] = fig
    print(f"[{side}] {name}: {fig}")


# ----------------------------------------------------------------------------------------------
# the assertions, as functions of "a rule's answers" so that the oracle, the device and the wrong rules go through the same ones
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def pairs_random():
    o, d, v = I.random_pairs()
    return o, d, v, R.edge_values(o, d, v[:, 0], v[:, 1], v[:, 2])


def assert_reference_cap(ev, what):
    share = float((R.classify(ev) == R.UNDECIDED).mean())
    assert share <= UNDECIDED_CAP, f"{what}: the reference leaves {share:.2%} of the pairs undecided"
    return share


def check_random_pairs(answers, what):
    o, d, v, ev = pairs_random()
    assert_reference_cap(ev, "random pairs")
    return R.check_pairs(ev, *answers, what)


@functools.lru_cache(None)
def pairs_dominant():
    o, d, v = I.dominant_axis_pairs()
    return o, d, v, R.edge_values(o, d, v[:, 0], v[:, 1], v[:, 2])


def check_swap_claim(plain, swapped, what):
    """hit, t bit for bit; u, v bit for bit up to the sign of an exact zero"""
    (h0, t0, u0, v0), (h1, t1, u1, v1) = plain, swapped
    assert np.array_equal(h0, h1), f"{what}: the hit decision depends on the kx/ky swap"
    h = h0
    assert np.array_equal(u32(t0[h]), u32(t1[h])), f"{what}: t depends on the kx/ky swap"
    for name, a, b in (("u", u0[h], u1[h]), ("v", v0[h], v1[h])):
        differ = u32(a) != u32(b)
        assert np.all((a[differ] == 0) & (b[differ] == 0)), f"{what}: a non-zero {name} depends on the kx/ky swap"
    return int((u32(u0[h]) != u32(u1[h])).sum() + (u32(v0[h]) != u32(v1[h])).sum())


@functools.lru_cache(None)
def zero_set():
    tris = I.grid_mesh()
    o, d, inc = I.exact_zero_rays(tris)
    n_vertex = sum(1 for k in range(len(o)) if np.all(o[k] + d[k] == np.round(o[k] + d[k])))
    po, pd = I.in_plane_rays()
    return tris, o, d, inc, n_vertex, po, pd


@functools.lru_cache(None)
def zero_reference():
    """edge_values of every exact-zero ray against its incident triangles (all of them through rationals: computed once)"""
    tris, o, d, inc, n_vertex, po, pd = zero_set()
    return [R.edge_values(o[i], d[i], tris[inc[i]][:, 0], tris[inc[i]][:, 1], tris[inc[i]][:, 2]) for i in range(len(o))]


# Two incident triangles of an edge-point ray each form t = fl(T^ * fl(1 / det^)) from their own T^ and det^. Were T^ / det^ the very same
# number for both, the two correctly rounded operations left over -- the reciprocal and the product -- would still put each t up to
# 2 * 2^-24 |t| away from it: 4 * 2^-24 |t| between the two is what consistent edge values allow, and what is asserted. (Vertex rays: 0.)
T_SPREAD = 4.0 * R.EPS


def t_spread(t):
    """largest difference among the T of one ray's incident hits, in units of 2^-24 |t|"""
    t = np.asarray(t, np.float64)
    return 0.0 if len(t) < 2 else float((t.max() - t.min()) / (R.EPS * np.abs(t).max()))


def check_exact_zeros(rule, what):
    """rule(o [3], d [3], tris [k, 3, 3]) -> hit [k], t [k]. Every ray hits an incident triangle; the incident hits of a vertex ray report
    the same T, those of an edge-point ray T within T_SPREAD of each other (and of the exact t within the t bound); rays in the plane hit
    nothing."""
    tris, o, d, inc, n_vertex, po, pd = zero_set()
    leaks, differ_vertex, differ_edge, off_bound, worst = 0, 0, 0, 0, 0.0
    for i in range(len(o)):
        tt = tris[inc[i]]
        hit, t = rule(o[i], d[i], tt)
        leaks += not hit.any()
        split = len(set(u32(t[hit]).tolist())) > 1
        if i < n_vertex:
            differ_vertex += split
        else:
            differ_edge += split
            worst = max(worst, t_spread(t[hit]))
            ev = zero_reference()[i]
            _, tb = R.bounds(ev)
            off_bound += int((np.abs(t[hit].astype(np.float64) - ev["t"][hit]) > tb[hit] * np.abs(ev["t"][hit])).sum())
    assert leaks == 0, f"{what}: {leaks} of {len(o)} rays through a vertex or an edge hit none of the incident triangles"
    assert differ_vertex == 0, f"{what}: {differ_vertex} of {n_vertex} vertex rays get different T from their incident triangles"
    assert worst <= T_SPREAD / R.EPS, f"{what}: incident triangles of an edge-point ray report T {worst:.2f} * 2^-24 |t| apart (allowed: {T_SPREAD / R.EPS:.0f})"
    assert off_bound == 0, f"{what}: {off_bound} edge-point hits report a T outside the t bound"
    in_plane = sum(int(rule(po[i], pd[i], tris)[0].sum()) for i in range(len(po)))
    assert in_plane == 0, f"{what}: {in_plane} hits reported for rays that travel in the triangles' plane (det = 0 exactly)"
    return {"rays": len(o), "leaks": leaks, "edge_rays_with_two_T": int(differ_edge), "edge_rays": len(o) - n_vertex,
            "worst_T_spread_in_eps": worst}


@functools.lru_cache(None)
def closed_sets():
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L
    import dxpbrt_amd.scenes as S

    class P:
        layouts, scenes = L, S
    return I.closed_mesh_sets(P, ge.load_oracle())


def check_closed(rec, expect, what):
    leak = rec["Instance"] != expect
    assert not leak.any(), (f"{what}: {int(leak.sum())} of {len(rec)} rays from inside a mesh leak (miss it or report another instance), "
                            f"first ray {int(np.nonzero(leak)[0][0])}")
    return int(leak.sum())


@functools.lru_cache(None)
def duplicate_set():
    import __graft_entry__ as ge
    ge.load_package()
    import dxpbrt_amd.layouts as L
    import dxpbrt_amd.scenes as S

    class P:
        layouts, scenes = L, S
    return I.duplicate_soup(P, ge.load_oracle())


def check_closest_of_many(rec, what):
    soup, rays = duplicate_set()
    fig = R.check_closest(rays, soup.instances, rec, soup.slot_of, what)
    want, copies = I.lowest_identical(soup, rec)
    got = np.stack([rec["Instance"], rec["Geometry"], rec["Primitive"]], 1).astype(np.int64)
    hit = rec["Instance"] != I.MISS
    bad = hit & (got != want).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} rays report a copy of their triangle that is not the lowest (instance, geometry, primitive), first ray {int(np.nonzero(bad)[0][0])}"
    fig["ties_settled"] = int((hit & (copies > 1)).sum())
    return fig


def interval_rays(rays, rec):
    """per hit ray six variants: tmin at T, below, above (tmax open) and tmax at T, below, above (tmin 0)"""
    hit = np.nonzero(rec["Instance"] != I.MISS)[0]
    T = rec["T"][hit]
    lo, hi = I.ulp_steps(T)
    out = np.repeat(rays[hit], 6, 0).reshape(len(hit), 6, 8)
    out[:, 0, 3], out[:, 1, 3], out[:, 2, 3] = T, lo, hi
    out[:, 3, 7], out[:, 4, 7], out[:, 5, 7] = T, lo, hi
    return hit, out.reshape(-1, 8)


def check_interval(rec0, hit, rec6, what):
    """rec0: the open-interval records; rec6: the records of interval_rays"""
    r = rec6.reshape(len(hit), 6)
    base = rec0[hit]
    same = lambda k: np.array([not I.same_records(r[i:i + 1, k], base[i:i + 1]) for i in range(len(hit))])
    T = base["T"]
    gone_min = (r[:, 0]["Instance"] == I.MISS) | (r[:, 0]["T"] > T)
    assert gone_min.all(), f"{what}: tmin = T keeps a hit at T on {int((~gone_min).sum())} rays (the interval is exclusive)"
    assert same(1).all(), f"{what}: tmin one ulp below T changes the record"
    gone = (r[:, 2]["Instance"] == I.MISS) | (r[:, 2]["T"] > T)
    assert gone.all(), f"{what}: tmin one ulp above T keeps the hit"
    assert (r[:, 3]["Instance"] == I.MISS).all(), f"{what}: tmax = T keeps the closest hit on {int((r[:, 3]['Instance'] != I.MISS).sum())} rays (the interval is exclusive)"
    assert (r[:, 4]["Instance"] == I.MISS).all(), f"{what}: tmax one ulp below T keeps a hit"
    assert same(5).all(), f"{what}: tmax one ulp above T changes the record"
    return {"rays": len(hit)}


# ----------------------------------------------------------------------------------------------
# CPU: the oracle
# ----------------------------------------------------------------------------------------------
def test_reference_alone_decides_nearly_everything():
    o, d, v, ev = pairs_random()
    share = assert_reference_cap(ev, "random pairs")
    assert int(ev["exact"].sum()) < len(o) // 100              # float64 decides; rationals are the exception
    tris, zo, zd, inc, n_vertex, po, pd = zero_set()
    leaks = 0
    for i in range(len(zo)):                                    # the reference's own watertightness: exact zeros count as inside
        ev1 = zero_reference()[i]
        assert ev1["exact"].all()                               # decided by rationals, every one of them
        leaks += not R.exact_hit(ev1).all()                     # EVERY incident triangle contains the point
    assert leaks == 0
    for i in range(len(po)):
        assert not R.exact_hit(R.edge_values(po[i], pd[i], tris[:, 0], tris[:, 1], tris[:, 2])).any()
    note("reference", "random pairs", {"undecided_share": share, "rational_rows": int(ev["exact"].sum())})
    note("reference", "exact zeros", {"rays": len(zo), "leaks": leaks})


def test_fma32_is_a_correctly_rounded_fma():
    """isectref.fma32 against exact rationals, on operands chosen to make the float64 sum land on fp32 ties"""
    from fractions import Fraction
    rng = np.random.default_rng(9)
    a = rng.normal(size=4000).astype(f32); b = rng.normal(size=4000).astype(f32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(f32) * f32(1 + 2.0 ** -12)       # heavy cancellation
    a[:64] = f32(1 + 2.0 ** -12); b[:64] = f32(1 + 2.0 ** -12); c[:64] = np.ldexp(f32(1.0), -np.arange(64, dtype=np.int32)).astype(f32) * f32(2.0 ** -1)
    got = R.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = f32(float(exact))                               # float(Fraction) rounds once to float64: repair as the function does is the point
        lo, hi = np.nextafter(near, f32(-np.inf)), np.nextafter(near, f32(np.inf))
        best = min((lo, near, hi), key=lambda x: (abs(Fraction(float(x)) - exact), int(u32(np.array([x], f32))[0]) & 1))
        assert u32(np.array([got[i]]))[0] == u32(np.array([best], f32))[0], i


def test_random_pairs_oracle(oracle):
    o, d, v, ev = pairs_random()
    hit, t, u, vv = I.oracle_pairs(oracle, o, d, v[:, 0], v[:, 1], v[:, 2])
    fig = check_random_pairs((hit, t, u, vv), "oracle")
    wh, wt, wu, wv, fb = R.woop_fp32(o, d, v[:, 0], v[:, 1], v[:, 2])
    assert np.array_equal(wh, hit) and all(np.array_equal(u32(a[hit]), u32(b[hit])) for a, b in ((wt, t), (wu, u), (wv, vv)))
    note("oracle", "random pairs", fig)


def test_dominant_axes_and_the_swap_oracle(oracle):
    o, d, v, ev = pairs_dominant()
    hit, t, u, vv = I.oracle_pairs(oracle, o, d, v[:, 0], v[:, 1], v[:, 2])
    wh, wt, wu, wv, fb = R.woop_fp32(o, d, v[:, 0], v[:, 1], v[:, 2])
    assert np.array_equal(wh, hit) and all(np.array_equal(u32(a[hit]), u32(b[hit])) for a, b in ((wt, t), (wu, u), (wv, vv)))
    assert int((fb & hit).sum()) >= 100                        # the hit rays include ones that take the fallback
    kz = R._dominant(d)
    for axis in range(3):
        for sign in (1, -1):
            sel = hit & (kz == axis) & (np.sign(d[np.arange(len(d)), kz]) == sign)
            assert sel.sum() >= 20 and (sel & fb).sum() >= 5, (axis, sign)
    a = np.abs(d)
    assert (hit & (a[:, 0] == a[:, 1])).sum() >= 20 and (hit & (a[:, 1] == a[:, 2])).sum() >= 20 and (hit & (a[:, 0] == a[:, 2])).sum() >= 20
    sh, st, su, sv, _ = R.woop_fp32(o, d, v[:, 0], v[:, 1], v[:, 2], paper_swap=True)
    zeros = check_swap_claim((hit, t, u, vv), (sh, st, su, sv), "dominant axes")
    assert zeros > 0                                            # the sign of a zero is where the two forms do differ: the claim is not vacuous
    fig = R.check_pairs(ev, hit, t, u, vv, "oracle, dominant axes")
    fig["zero_signs_the_swap_flips"] = zeros
    note("oracle", "dominant axes", fig)


def test_exact_zeros_oracle(oracle):
    """The same T is asserted for the integer rays through vertices, where the sheared vertex is exactly (0, 0). A ray through a quarter
    point of an edge gets t as the U : V weighted mean of two vertex depths times fl(1 / det), from each triangle's own U, V and det: the
    incident hits must agree within T_SPREAD = 4 * 2^-24 |t| (see there; oracle and MI355X: 13 of 1 536 such rays report two T, at most
    3 * 2^-24 |t| apart) and with the exact t within the t bound."""
    def rule(o, d, tt):
        hit, t, _, _ = I.oracle_pairs(oracle, o, d, tt[:, 0], tt[:, 1], tt[:, 2])
        return hit, t
    note("oracle", "exact zeros", check_exact_zeros(rule, "oracle"))


def test_closed_meshes_oracle(oracle):
    total = 0
    for name, soup, rays, expect in closed_sets():
        rec = I.oracle_closest(oracle, soup.scene, rays)
        check_closed(rec, expect, f"oracle, {name}")
        vis = I.oracle_visibility(oracle, soup.scene, rays)
        assert (vis[:, 3] == 0).all(), f"oracle, {name}: {int((vis[:, 3] != 0).sum())} rays from inside a mesh are unoccluded"
        again = I.oracle_closest(oracle, soup.scene, rays, accel_mode=1)          # the oracle's own BVH must not lose a hit either
        assert not I.same_records(again, rec), name
        total += len(rays)
    note("oracle", "closed meshes", {"rays": total, "leaks": 0})


def test_closed_meshes_against_the_exact_closest(oracle):
    """closest-of-many by the exact reference on the meshes of up to 320 triangles, every placement (each mesh against its own rays)"""
    worst, und, pairs = {"u": 0.0, "v": 0.0, "t": 0.0}, 0, 0
    for name, soup, rays, expect in closed_sets():
        rec = I.oracle_closest(oracle, soup.scene, rays)
        for x in range(len(soup.instances)):
            if len(soup.instances[x][1]) > 320:
                continue
            sel = np.nonzero(expect == x)[0][::3]
            fig = R.check_closest(rays[sel], soup.only(x), rec[sel], soup.slot_of, f"oracle, {name}, instance {x}")
            for k in worst:
                worst[k] = max(worst[k], fig[k])
            und += fig["undecided_pairs"]; pairs += len(sel) * len(soup.instances[x][1])
    worst["undecided_share"] = und / pairs
    note("oracle", "closed meshes, exact closest", worst)


def test_closest_of_many_oracle(oracle):
    soup, rays = duplicate_set()
    rec = I.oracle_closest(oracle, soup.scene, rays)
    fig = check_closest_of_many(rec, "oracle")
    assert fig["hits"] > len(rays) // 2 and fig["ties_settled"] > 50
    note("oracle", "closest of many", fig)


def test_interval_rule_oracle(oracle):
    soup, rays = duplicate_set()
    rec0 = I.oracle_closest(oracle, soup.scene, rays)
    hit, six = interval_rays(rays, rec0)
    note("oracle", "interval rule", check_interval(rec0, hit, I.oracle_closest(oracle, soup.scene, six), "oracle"))


# ----------------------------------------------------------------------------------------------
# wrong rules
# ----------------------------------------------------------------------------------------------
def _pair_rule(wrong):
    def rule(o, d, tt):
        hit, t, _, _, _ = R.woop_fp32(o, d, tt[:, 0], tt[:, 1], tt[:, 2], wrong)
        return hit, t
    return rule


def _wrong_random(wrong):
    o, d, v, ev = pairs_random()
    check_random_pairs(R.woop_fp32(o, d, v[:, 0], v[:, 1], v[:, 2], wrong)[:4], wrong)


def _wrong_zeros(wrong):
    check_exact_zeros(_pair_rule(wrong), wrong)


def _wrong_closed(wrong):
    import __graft_entry__ as ge
    for name, soup, rays, expect in closed_sets():
        ref = I.oracle_closest(ge.load_oracle(), soup.scene, rays)
        for x in range(len(soup.instances)):                    # each mesh against its own rays: a hit elsewhere would be a leak anyway
            sel = expect == x
            rec = R.woop_closest(rays[sel], soup.only(x), wrong)
            check_closed(rec, expect[sel], f"{wrong}, {name}, instance {x}")
            bad = I.same_records(rec, ref[sel])                 # what device_records asks of the device
            assert not bad, f"{wrong}, {name}, instance {x}: the rule and the oracle differ: {bad}"


def _wrong_closest(wrong):
    soup, rays = duplicate_set()
    check_closest_of_many(R.woop_closest(rays, soup.instances, wrong), wrong)


def _wrong_interval(wrong):
    soup, rays = duplicate_set()
    rec0 = R.woop_closest(rays, soup.instances, wrong)
    hit, six = interval_rays(rays, rec0)
    check_interval(rec0, hit, R.woop_closest(six, soup.instances, wrong), wrong)


# wrong rule -> (the input set it must fail on, a phrase of the assertion that must catch it)
WRONG_RULE_BREAKS = {
    "no_fallback": (_wrong_closed, "the rule and the oracle differ"),     # it cannot leak (a zero edge value counts as inside): it reports the
                                                                         # triangle across the edge instead, which only the bit comparison sees
    "fma_edges": (_wrong_zeros, "hit none of the incident triangles"),
    "fixed_kz": (_wrong_random, "outside the derived bound"),
    "accept_det0": (_wrong_zeros, "travel in the triangles' plane"),
    "swap_uv": (_wrong_random, "u outside the derived bound"),
    "cull_back": (_wrong_random, "classification differs"),
    "inclusive_tmin": (_wrong_interval, "tmin = T keeps a hit"),
    "last_tie": (_wrong_closest, "not the lowest"),
}


def test_the_right_rule_passes_where_the_wrong_ones_must_fail():
    """woop_fp32 / woop_closest without a wrong switch go through every check the wrong rules are held against (and equal the oracle: the
    tests above), so a failure below is the wrong rule's, not the restatement's."""
    for run in {f for f, _ in WRONG_RULE_BREAKS.values()}:
        run(None)


@pytest.mark.parametrize("wrong", R.WRONG_RULES)
def test_wrong_rule_breaks_its_assertion(wrong):
    run, phrase = WRONG_RULE_BREAKS[wrong]
    with pytest.raises(AssertionError) as e:
        run(wrong)
    assert phrase in str(e.value), f"{wrong} failed another assertion than the one named for it: {e.value}"


# ----------------------------------------------------------------------------------------------
# GPU: the kernels
# ----------------------------------------------------------------------------------------------
device_records = I.device_records


@pytest.fixture(scope="module")
def pair_soups(pkg, oracle):
    """the pairs as one bottom level each (a ray sees every triangle of its set: the record is the closest of them)"""
    out = {}
    for name, (o, d, v, ev) in (("random", pairs_random()), ("dominant", pairs_dominant())):
        with np.errstate(invalid="ignore"):
            own = R.exact_hit(ev) & (ev["t"] > 0)                 # an interval around the ray's own triangle keeps most others out of it
            tmin, tmax = np.where(own, ev["t"] * 0.875, 0.0).astype(f32), np.where(own, ev["t"] * 1.125, np.inf).astype(f32)
        out[name] = (I.Soup(pkg, oracle, [[v]], [(0, I.identity())]), I.rays_of(o, d, tmin, tmax))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "dominant"])
def test_pairs_gpu(gpu, ptamd, oracle, pair_soups, name):
    soup, rays = pair_soups[name]
    ref = I.oracle_closest(oracle, soup.scene, rays)
    rec = device_records(gpu, ptamd, soup, rays, name, ref)
    own = (rec["Instance"] == 0) & (rec["Primitive"] == np.arange(len(rays)))
    ev = (pairs_random() if name == "random" else pairs_dominant())[3]
    inside = (R.classify(ev) == R.INSIDE) & (ev["t"] > 0)
    assert own.sum() >= inside.sum() // 2                       # the set is about the pairs: most rays that hit their own triangle report it
    fig = R.check_closest(rays, soup.instances, rec, soup.slot_of, f"device, {name} pairs", all_pairs=False, candidates=np.arange(len(rays)))
    fig["own_triangle"] = int(own.sum())
    note("device", f"{name} pairs", fig)


@pytest.mark.gpu
def test_exact_zeros_gpu(gpu, ptamd, oracle, pkg):
    """The closest-hit entry reports one triangle per ray, so the other incident hits are drawn out one by one: the ray again with tmin at
    the T just reported (exclusive: triangles at that very T drop out together), until it misses. The plane is crossed once, so every hit
    is an incident triangle; a vertex ray must miss at the second go, an edge-point ray's last T lies within T_SPREAD of its first."""
    tris, o, d, inc, n_vertex, po, pd = zero_set()
    soup = I.Soup(pkg, oracle, [[tris]], [(0, I.identity())])
    rays = np.concatenate([I.rays_of(o, d), I.rays_of(po, pd)])
    ref = I.oracle_closest(oracle, soup.scene, rays)
    rec = device_records(gpu, ptamd, soup, rays, "exact zeros", ref)
    hit = rec["Instance"] != I.MISS
    assert hit[:len(o)].all(), f"{int((~hit[:len(o)]).sum())} rays through a vertex or an edge leak"
    assert not hit[len(o):].any(), "a ray in the plane of the mesh reports a hit"
    assert all(rec["Primitive"][i] in inc[i] for i in range(len(o)))
    assert np.array_equal(rec["T"][:n_vertex], np.ones(n_vertex, f32))           # the aimed point is o + d
    first = rec["T"][:len(o)].astype(np.float64); last = first.copy()
    live = np.arange(len(o)); again = rays[:len(o)].copy(); rounds = 0
    while len(live):
        again[live, 3] = last[live].astype(f32)
        nxt = device_records(gpu, ptamd, soup, again[live], "exact zeros, next hit", I.oracle_closest(oracle, soup.scene, again[live]))
        more = nxt["Instance"] != I.MISS
        assert all(nxt["Primitive"][k] in inc[live[k]] for k in np.nonzero(more)[0])
        assert not more[live < n_vertex].any(), f"{int(more[live < n_vertex].sum())} vertex rays get a second T from their incident triangles"
        last[live[more]] = nxt["T"][more]
        live = live[more]; rounds += 1
        assert rounds <= 6                                      # six triangles meet at a vertex at the most
    spread = (last - first) / (R.EPS * np.abs(last))
    assert spread.max() <= T_SPREAD / R.EPS, f"incident triangles of an edge-point ray report T {spread.max():.2f} * 2^-24 |t| apart"
    note("device", "exact zeros", {"rays": len(o), "leaks": int((~hit[:len(o)]).sum()), "edge_rays_with_two_T": int((spread > 0).sum()),
                                   "worst_T_spread_in_eps": float(spread.max())})


@pytest.mark.gpu
def test_closed_meshes_gpu(gpu, ptamd, oracle):
    import torch
    import ctypes as C
    total = 0
    for name, soup, rays, expect in closed_sets():
        ref = I.oracle_closest(oracle, soup.scene, rays)
        rec = device_records(gpu, ptamd, soup, rays, name, ref)
        check_closed(rec, expect, f"device, {name}")
        g = ptamd.Scene(gpu, soup.scene)
        try:
            dr = torch.from_numpy(rays).cuda(); dv = torch.zeros((len(rays), 4), dtype=torch.float32, device="cuda")
            gpu.check(gpu.lib.pt_trace_visibility(gpu.handle, C.c_void_p(dr.data_ptr()), len(rays), C.c_void_p(dv.data_ptr())))
            gpu.sync()
            vis = dv.cpu().numpy()
        finally:
            g.close()
        assert (vis[:, 3] == 0).all(), f"device, {name}: the any-hit walk leaves {int((vis[:, 3] != 0).sum())} rays from inside a mesh unoccluded"
        total += len(rays)
    note("device", "closed meshes", {"rays": total, "leaks": 0})


@pytest.mark.gpu
def test_closest_interval_and_launch_shape_gpu(gpu, ptamd, oracle):
    soup, rays = duplicate_set()
    ref = I.oracle_closest(oracle, soup.scene, rays)
    rec = device_records(gpu, ptamd, soup, rays, "closest of many", ref)
    note("device", "closest of many", check_closest_of_many(rec, "device"))
    hit, six = interval_rays(rays, rec)
    rec6 = device_records(gpu, ptamd, soup, six, "interval rule", I.oracle_closest(oracle, soup.scene, six))
    note("device", "interval rule", check_interval(rec, hit, rec6, "device"))
    big = np.tile(rays, (20001 // len(rays) + 1, 1))[:20001]
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, soup.scene)
    try:
        whole = gpu.trace_closest(big)
        assert not I.same_records(whole, np.tile(rec, 20001 // len(rays) + 1)[:20001], I.FIELDS + ("Slot",))
        for n in (1, 63, 64, 65, 257):
            for brute in (False, True):
                part = gpu.trace_closest(big[:n], brute_force=brute)
                assert not I.same_records(part, whole[:n], I.FIELDS + ("Slot",)), (n, brute)
    finally:
        g.close()
