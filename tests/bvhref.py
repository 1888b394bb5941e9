"""An independent restatement of the tree the device builder (csrc/pt_bvh.hip) must choose, and the checks a downloaded tree has to pass.

bvh_check.check_blob asks whether a tree is VALID. Any valid tree renders the same image, so a builder that keys, sorts, collapses or
quantises wrongly stays green there. This module states the builder's rules a second time, in numpy and plain Python, from nothing
but the inputs the traversal copy (pt_debug_download_blob) holds, and demands the device's tree to be THE tree of those rules:

  items      one fp32 box per item in API order. Bottom level: the box of each packet's three vertices, ordered by geometry, then
             primitive. Top level: the world box of each instance as k_instance_boxes computes it (instance_boxes() below).
             NOTE: the instance records of the copy do NOT hold these boxes. k_blob_assemble runs pad_box over them first, while
             k_morton keys, and k_leaves bounds, with the unpadded ones (padding moves the scene bounds by 1e-5 of the coordinates:
             some twenty Morton cells). So the boxes are restated from the transforms, the packets and the bottom level's root box,
             and the records' boxLo / boxHi serve as a witness: pad_box of the restated box must equal them bit for bit.
  order      scene bounds, box centre and the 21-bit cell per axis in float32 with the operations of k_morton one by one, bit
             interleave (x highest), for a top level `>> 3` and bit 62 for an item that spans more than large_fraction of the scene along an
             axis, stable sort by key. Exact integers.
  binary     leaves of leaf_size consecutive sorted items keyed by their first item; the radix tree over (key, position): a range is
             split at the highest bit in which its first and last key differ, a range of equal keys at the highest bit in which its
             first and last POSITION differ. Built top-down by that sentence (the device runs Karras' per-node searches). Exact.
  boxes      pad_box in float32 on every leaf's union box, min / max up the tree. Order-independent, exact.
  collapse   cost tables in float64: C(n, i) = cheapest cost of binary node n as a forest of at most i roots,
                 C(n, 1) = min(C_leaf, C_node),  C_leaf = A P c_item  (P <= max_leaf_items),  C_node = A c_node + D(n, 8)
                 C(n, i) = min(D(n, i), C(n, i - 1)),   D(n, j) = min over 0 < k < j of C(left, k) + C(right, j - k)
             A the half area (0 for an empty or non-finite box), P the items below n. A tree of two or more leaves starts at a wide node
             whatever its size (the traversal enters a node), so the optimum of a tree is C_node(root), not C(root, 1).
  slots      the greedy (child, slot) assignment of collapse_node step 3 in float32: cost of child c in slot s is the sum over the
             axes of +-d, d the child's centre minus the node's, minus where the slot's bit of that axis (x: 4, y: 2, z: 1) is
             set; per round every unassigned child names its cheapest free slot (the lowest such), the cheapest child wins, equal costs
             go to the lower rank (left-to-right position), then the lower slot.
  quantise   origin = the node's low corner; per axis the least e >= -126 with every child's high side within 255 * 2^e of the
             origin (-126 for a zero extent); q_lo the largest, q_hi the smallest byte whose decoded plane, fp32(origin + q 2^e) as
             wide_child_box decodes it, is on the outer side of the child's box.

check_tree() / check() take the parts to be asked as a string of letters:
  a  membership: the items below every occupied slot are exactly the items of one binary node; a leaf slot is a whole subtree of at
     most max_leaf_items items; the slots of a node tile its own binary node. No tolerance.
  b  order: within a leaf slot the items stand in sorted order; a node's leaf items follow each other from triBase in slot order.
  c  optimality: cost(device tree) <= optimum (1 + eps), both float64 in the model above,
         eps = 2 (2 H + 8) 2^-24,   H the height of the binary tree.
     Derivation: every term of the device's fp32 tables is non-negative, so roundings only accumulate relatively. A half area is
     three differences, three products and two sums: at most 5 roundings on a path; a leaf cost adds 2 products, a node's own term 1:
     8 in all. Every level of the binary tree adds one sum for D and one for A c_node + D(n, 8): 2 H. An entry of a table is thus
     within (1 +- u)^(2 H + 8), u = 2^-24, of its float64 value. The device takes minima among such entries, so the tree it reads off
     the tables costs, in its own arithmetic, no more than the optimum does in its own arithmetic: a factor (1 + u)^(2 H + 8) on
     either side, hence 2 (2 H + 8) u to first order (the second order is below 1e-10 for H < 64). A decision taken from a stale or
     misread table is off by percents.
  d  origin bit for bit; the exponent rule above: at the stored e the decoded plane 255 reaches the farthest child, at e - 1 the fit,
     re-run in exact rational arithmetic, overflows; -126 on zero-extent axes; empty slots [255, 0] with meta 0.
  e  boxes: with D = fp32(origin + q 2^e), D_lo <= lo and D_hi >= hi of the PADDED binary box of the slot (containment), and
     lo - D_lo, D_hi - hi <= 2^e + 2^-24 max(|D|, |coordinate|) (tightness: one quantum plus one fp32 rounding of the coordinate,
     which covers the device's fp32 post-correction p + q scale).
  f  slots: every child sits in the slot the restated greedy rule gives it; imask, meta and the rank order of childBase agree.
  g  counts for the header facts: nodes and depth of the walked tree (check() holds them against accel_stats()).
"""
from fractions import Fraction

import numpy as np

import bvh_check

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


class Params:
    """what build_bottom_level / build_top_level hand to build_wide_tree; the test modules state the values"""

    def __init__(self, leaf_size, max_leaf_items, cost_item, cubic, large_first, cost_node=1.0, large_fraction=0.25):
        self.leaf_size, self.max_leaf_items = int(leaf_size), int(max_leaf_items)
        self.cost_item, self.cost_node = float(f32(cost_item)), float(f32(cost_node))       # the device holds them as fp32 constants
        self.cubic, self.large_first, self.large_fraction = bool(cubic), bool(large_first), f32(large_fraction)


def eps_of(height):
    return 2.0 * (2.0 * height + 8.0) * U


# ---------------------------------------------------------------------------------------------
# items, keys, order
# ---------------------------------------------------------------------------------------------
def triangle_boxes(tris):
    """tris: bvh_check.TRI_DT packets of one bottom level in any order -> (lo, hi) [n, 3] float32 in API order (geometry, then primitive),
    and api_of_packet [n]: the API index of every packet"""
    g, p = tris["geom"].astype(np.int64), tris["prim"].astype(np.int64)
    counts = np.zeros(int(g.max()) + 1 if len(g) else 0, np.int64)
    if len(g):
        np.maximum.at(counts, g, p + 1)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    api = offsets[g] + p
    assert len(np.unique(api)) == len(tris) and (not len(api) or api.max() == len(tris) - 1), "the packets are not one per (geometry, primitive)"
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], 1)
    lo, hi = np.empty((len(tris), 3), f32), np.empty((len(tris), 3), f32)
    lo[api], hi[api] = v.min(1), v.max(1)
    return lo, hi, api


def pad_boxes(lo, hi):
    """pad_box, per axis with lo <= hi: e = 1e-5 max(|lo|, |hi|) + 1e-6 (hi - lo) + 1e-30, float32, in that order"""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    with np.errstate(all="ignore"):
        e = (f32(1e-5) * np.maximum(np.abs(lo), np.abs(hi)) + f32(1e-6) * (hi - lo)) + f32(1e-30)
        ok = lo <= hi
        return np.where(ok, lo - e, lo).astype(f32), np.where(ok, hi + e, hi).astype(f32)


def scene_bounds(lo, hi):
    """per axis over the items whose box is not inverted on that axis; NaN where there is none (the device's untouched atomics decode to NaN)"""
    mn, mx = np.full(3, np.nan, f32), np.full(3, np.nan, f32)
    for a in range(3):
        ok = lo[:, a] <= hi[:, a]
        if ok.any():
            mn[a], mx[a] = lo[ok, a].min(), hi[ok, a].max()
    return mn, mx


def morton_keys(lo, hi, P):
    """-> (keys as uint64 [n], large [n] bool)"""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    mn, mx = scene_bounds(lo, hi)
    with np.errstate(all="ignore"):
        ext0 = (mx - mn).astype(f32)
        ext = np.full(3, np.fmax(ext0[0], np.fmax(ext0[1], ext0[2])), f32) if P.cubic else ext0
        c = (f32(0.5) * (lo + hi)).astype(f32)
        f = np.where(ext > 0, ((c - mn).astype(f32) / ext).astype(f32), f32(0)).astype(f32)
        f = np.where(np.isnan(f), f32(0), f)
        cell = np.minimum(np.maximum((f * f32(2097152.0)).astype(f32), f32(0)), f32(2097151.0)).astype(np.uint64)
        span = (hi - lo).astype(f32)
        large = ((ext0 > 0) & (span > (P.large_fraction * ext0).astype(f32))).any(1)
    keys = np.zeros(len(lo), np.uint64)
    for b in range(21):
        for a in range(3):                                # x above y above z within every triple of bits
            keys |= ((cell[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    if P.large_first:
        keys = (keys >> np.uint64(3)) | (large.astype(np.uint64) << np.uint64(62))
    else:
        large = np.zeros(len(lo), bool)
    return keys, large


def radix_tree(keys):
    """keys: sorted. -> first, last (leaf range, inclusive), left, right per internal node; node 0 is the root, a child < 0 is leaf ~child.
    Children are created after their parents, so descending node order is a bottom-up order."""
    K = [int(k) for k in keys]
    Knp = np.asarray(keys, np.uint64)
    first, last, left, right = [], [], [], []

    def new(a, b):
        first.append(a); last.append(b); left.append(0); right.append(0)
        return len(first) - 1
    if len(K) < 2:
        return first, last, left, right
    stack = [new(0, len(K) - 1)]
    while stack:
        i = stack.pop()
        a, b = first[i], last[i]
        if K[a] != K[b]:
            bit = (K[a] ^ K[b]).bit_length() - 1
            s = a + int(np.searchsorted(Knp[a:b + 1], np.uint64((K[b] >> bit) << bit), "left"))
        else:
            bit = (a ^ b).bit_length() - 1
            s = (b >> bit) << bit
        assert a < s <= b
        for side, (x, y) in enumerate(((a, s - 1), (s, b))):
            ref = ~x if x == y else new(x, y)
            if ref >= 0:
                stack.append(ref)
            (right if side else left)[i] = ref
    return first, last, left, right


def half_area(lo, hi):
    d = [float(hi[a]) - float(lo[a]) for a in range(3)]
    with np.errstate(all="ignore"):
        a = d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    return a if a == a and d[0] >= 0.0 else 0.0


class Tree:
    """the restated order, binary tree, boxes and cost tables of one set of items"""

    def __init__(self, lo, hi, P, keys_hook=None, order_hook=None, unpad_leaf=None, stale=None):
        self.P, self.n = P, len(lo)
        self.item_lo, self.item_hi = np.asarray(lo, f32).reshape(-1, 3), np.asarray(hi, f32).reshape(-1, 3)
        self.keys, self.large = morton_keys(self.item_lo, self.item_hi, P)
        if keys_hook:
            self.keys = keys_hook(self.keys.copy())
        self.order = np.argsort(self.keys, kind="stable")               # order[sorted position] = item
        self.sorted_keys = self.keys[self.order]
        if order_hook:
            self.order = order_hook(self.order.copy())
        self.pos_of_item = np.empty(self.n, np.int64); self.pos_of_item[self.order] = np.arange(self.n)
        L = P.leaf_size
        self.nleaves = (self.n + L - 1) // L
        self.leaf_count = [min(L, self.n - l * L) for l in range(self.nleaves)]
        self.first, self.last, self.left, self.right = radix_tree(self.sorted_keys[::L])
        self.range_to_ref = {(l, l): ~l for l in range(self.nleaves)}
        for i in range(len(self.first)):
            self.range_to_ref[(self.first[i], self.last[i])] = i
        self.height = 0
        h = [0] * len(self.first)
        for i in reversed(range(len(self.first))):
            h[i] = 1 + max(h[self.left[i]] if self.left[i] >= 0 else 0, h[self.right[i]] if self.right[i] >= 0 else 0)
        self.height = h[0] if h else 0
        self.rebox(self.item_lo, self.item_hi, unpad_leaf)
        self.tables(stale)

    def rebox(self, lo, hi, unpad_leaf=None):
        """boxes of the same topology over other item boxes (a refit)"""
        lo, hi = np.asarray(lo, f32).reshape(-1, 3), np.asarray(hi, f32).reshape(-1, 3)
        L, nl = self.P.leaf_size, self.nleaves
        slo, shi = lo[self.order], hi[self.order]
        padn = nl * L - self.n
        if padn:
            slo = np.concatenate([slo, np.full((padn, 3), np.inf, f32)]); shi = np.concatenate([shi, np.full((padn, 3), -np.inf, f32)])
        ulo, uhi = slo.reshape(nl, L, 3).min(1) if nl else slo, shi.reshape(nl, L, 3).max(1) if nl else shi
        self.leaf_lo, self.leaf_hi = pad_boxes(ulo, uhi)
        if unpad_leaf is not None:
            self.leaf_lo[unpad_leaf], self.leaf_hi[unpad_leaf] = ulo[unpad_leaf], uhi[unpad_leaf]
        ni = len(self.first)
        self.node_lo, self.node_hi = np.empty((ni, 3), f32), np.empty((ni, 3), f32)
        self.node_items = [0] * ni
        for i in reversed(range(ni)):
            l, r = self.left[i], self.right[i]
            self.node_lo[i] = np.minimum(self.box(l)[0], self.box(r)[0]); self.node_hi[i] = np.maximum(self.box(l)[1], self.box(r)[1])
            self.node_items[i] = self.items(l) + self.items(r)
        return self

    def box(self, ref):
        return (self.leaf_lo[~ref], self.leaf_hi[~ref]) if ref < 0 else (self.node_lo[ref], self.node_hi[ref])

    def items(self, ref):
        return self.leaf_count[~ref] if ref < 0 else self.node_items[ref]

    def leaf_range(self, ref):
        return (~ref, ~ref) if ref < 0 else (self.first[ref], self.last[ref])

    def root_bounds(self):
        """lo.xyz hi.xyz the build leaves as the bottom level's root bounds"""
        if self.n == 0:
            return np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
        return self.box(~0 if self.nleaves == 1 else 0)

    def area(self, ref):
        return half_area(*self.box(ref))

    def leaf_cost(self, ref):
        return self.area(ref) * self.items(ref) * self.P.cost_item

    def tables(self, stale=None):
        """cost[n][i - 1] = C(n, i), split[n][j] = k of the best distribution over j roots (0: take C(n, j - 1)), is_leaf[n]. Ties go to
        more roots and to the lower k, as on the device (any other rule gives the same costs). stale: a node whose table reads as
        zeros when its parent decides (what a read before the writer's store arrived looks like)."""
        ni = len(self.first)
        self.cost, self.split, self.is_leaf, self.dist8 = [None] * ni, [None] * ni, [False] * ni, [0.0] * ni
        inf = float("inf")
        for n in reversed(range(ni)):
            c = []
            for r in (self.left[n], self.right[n]):
                c.append([self.leaf_cost(r)] * 7 if r < 0 else ([0.0] * 7 if r == stale else self.cost[r]))
            dist, split = [inf] * 9, [0] * 9
            for j in range(2, 9):
                for k in range(max(1, j - 7), min(7, j - 1) + 1):
                    v = c[0][k - 1] + c[1][j - k - 1]
                    if v < dist[j]:
                        dist[j], split[j] = v, k
            A, Pn = self.area(n), self.node_items[n]
            c_leaf = A * Pn * self.P.cost_item if Pn <= self.P.max_leaf_items else inf
            c_node = A * self.P.cost_node + dist[8]
            self.is_leaf[n] = c_leaf <= c_node
            cost = [min(c_leaf, c_node)]
            for i in range(2, 8):
                if dist[i] <= cost[-1]:
                    cost.append(dist[i])
                else:
                    cost.append(cost[-1]); split[i] = 0
            self.cost[n], self.split[n], self.dist8[n] = cost, split, dist[8]
        self.optimum = self.area(0) * self.P.cost_node + self.dist8[0] if ni else 0.0

    def expand(self, root, force=None):
        """the children the tables give the wide node grown from binary node `root`: [(ref, is a leaf slot)] from left to right.
        force: {(binary node, roots): k} replaces single decisions (a legal distribution, not the cheapest)."""
        out = []

        def rec(ref, budget, top):
            if ref < 0:
                out.append((ref, True)); return
            if not top:
                while budget > 1 and self.split[ref][budget] == 0:
                    budget -= 1
            if budget == 1:
                out.append((ref, bool(self.is_leaf[ref]))); return
            k = (force or {}).get((ref, budget), self.split[ref][budget])
            assert 1 <= k <= 7 and 1 <= budget - k <= 7
            rec(self.left[ref], k, False); rec(self.right[ref], budget - k, False)
        rec(root, 8, True)
        return out

    def greedy_cost(self):
        """the cost of the collapse that opens the child of the largest area until eight stand (and makes a leaf of nothing but a binary
        leaf): what the builder did before the tables. Legal, so the optimum cannot exceed it."""
        total, stack = 0.0, [0] if self.first else []
        while stack:
            n = stack.pop()
            total += self.area(n) * self.P.cost_node
            kids = [self.left[n], self.right[n]]
            while len(kids) < 8 and any(k >= 0 for k in kids):
                j = max((k for k in range(len(kids)) if kids[k] >= 0), key=lambda k: self.area(kids[k]))
                kids[j:j + 1] = [self.left[kids[j]], self.right[kids[j]]]
            for k in kids:
                if k < 0:
                    total += self.leaf_cost(k)
                else:
                    stack.append(k)
        return total


def slot_rule(node_lo, node_hi, child_lo, child_hi):
    """child_*: [n, 3] float32 in left-to-right order -> the slot of every child"""
    n = len(child_lo)
    with np.errstate(all="ignore"):
        c = (f32(0.5) * (np.asarray(node_lo, f32) + np.asarray(node_hi, f32))).astype(f32)
        d = ((f32(0.5) * (np.asarray(child_lo, f32) + np.asarray(child_hi, f32))).astype(f32) - c).astype(f32)
    d = np.where(np.isnan(d), f32(0), d).astype(f32)
    cost = np.empty((n, 8), f32)
    for s in range(8):
        sx, sy, sz = (-d[:, 0] if s & 4 else d[:, 0]), (-d[:, 1] if s & 2 else d[:, 1]), (-d[:, 2] if s & 1 else d[:, 2])
        cost[:, s] = ((sx + sy).astype(f32) + sz).astype(f32)
    free, slots = list(range(8)), [None] * n
    for _ in range(n):
        best = None
        for r in range(n):
            if slots[r] is not None:
                continue
            s = min(free, key=lambda s: (cost[r, s], s))
            cand = (cost[r, s], r, s)
            if best is None or cand < best:
                best = cand
        slots[best[1]] = best[2]; free.remove(best[2])
    return slots


def fits(origin, hi_max, e):
    """exact: does the farthest high side lie within 255 quanta 2^e of the origin?"""
    return Fraction(float(hi_max)) - Fraction(float(origin)) <= 255 * Fraction(2) ** e


def least_exponent(origin, hi_max):
    if not float(hi_max) > float(origin):
        return -126
    e = -126
    while not fits(origin, hi_max, e):
        e += 1
    return e


def decode(origin, q, e):
    """fp32(origin + q 2^e) (q 2^e is exact in fp32), as wide_child_box decodes a plane"""
    with np.errstate(all="ignore"):
        return (f32(origin) + (f32(q) * f32(np.ldexp(1.0, int(e)))).astype(f32)).astype(f32)


# ---------------------------------------------------------------------------------------------
# the restatement's own tree as node records
# ---------------------------------------------------------------------------------------------
def build(lo, hi, P, keys_hook=None, order_hook=None, unpad_leaf=None, stale=None, force=None, swap_slots=None):
    """-> (nodes as bvh_check.NODE_DT in breadth-first allocation order, item_of_position [n]: the API item at every position of the
    node-ordered item array, Tree, slot_of_position [n]: 8 * node + slot of the leaf slot holding every position).
    The hooks damage ONE rule on the way and leave a valid tree behind (tests/test_bvh_builder_rules.py): keys_hook(keys) -> keys before the
    sort, order_hook(order) -> order after it, unpad_leaf: a leaf whose box stays unpadded, stale / force: see Tree.tables / Tree.expand,
    swap_slots: (node, rank i, rank j) exchanges the slots of two children."""
    T = Tree(lo, hi, P, keys_hook, order_hook, unpad_leaf, stale)
    if T.nleaves <= 1:
        nodes = np.zeros(1, bvh_check.NODE_DT)
        for a in "xyz":
            nodes["qlo" + a] = 255
        nodes["exp"] = 1
        return nodes, T.order.copy(), T, np.zeros(T.n, np.int64)
    recs, roots, item_of_position, slot_of_position = [], [0], [], []
    w = 0
    while w < len(roots):
        root = roots[w]
        kids = T.expand(root, force)
        nlo, nhi = T.box(root)
        clo, chi = np.array([T.box(r)[0] for r, _ in kids]), np.array([T.box(r)[1] for r, _ in kids])
        slots = slot_rule(nlo, nhi, clo, chi)
        if swap_slots and swap_slots[0] == w:
            i, j = swap_slots[1:]
            slots[i], slots[j] = slots[j], slots[i]
        rec = np.zeros((), bvh_check.NODE_DT)
        valid = bool((nlo <= nhi).all() and np.isfinite(nlo).all() and np.isfinite(nhi).all())
        rec["origin"] = nlo if valid else 0
        rec["childBase"], rec["triBase"] = len(roots), len(item_of_position)
        for a in "xyz":
            rec["qlo" + a] = 255
        by_slot = sorted(range(len(kids)), key=lambda k: slots[k])
        ti = 0
        for k in by_slot:
            (ref, leaf), s = kids[k], slots[k]
            if leaf:
                a, b = T.leaf_range(ref)
                cnt = T.items(ref)
                rec["meta"][s] = (((1 << cnt) - 1) << 5) | ti
                p0 = a * P.leaf_size
                slot_of_position += [8 * w + s] * cnt
                item_of_position += T.order[p0:p0 + cnt].tolist()
                ti += cnt
            else:
                rec["meta"][s] = 0x20 | (24 + s)
                rec["imask"] |= 1 << s
                roots.append(ref)
        assert ti <= 24
        for a in range(3):
            ax = "xyz"[a]
            boxed = [k for k in range(len(kids)) if valid and clo[k, a] <= chi[k, a]]
            e = least_exponent(nlo[a], max([chi[k, a] for k in boxed], default=nlo[a])) if valid else -126
            rec["exp"][a] = e + 127
            for k in boxed:
                ql = int(np.clip(np.floor((float(clo[k, a]) - float(nlo[a])) / np.ldexp(1.0, e)), 0, 255))
                while ql > 0 and decode(nlo[a], ql, e) > clo[k, a]:
                    ql -= 1
                while ql < 255 and decode(nlo[a], ql + 1, e) <= clo[k, a]:
                    ql += 1
                qh = int(np.clip(np.ceil((float(chi[k, a]) - float(nlo[a])) / np.ldexp(1.0, e)), 0, 255))
                while qh < 255 and decode(nlo[a], qh, e) < chi[k, a]:
                    qh += 1
                while qh > 0 and decode(nlo[a], qh - 1, e) >= chi[k, a]:
                    qh -= 1
                rec["qlo" + ax][slots[k]], rec["qhi" + ax][slots[k]] = ql, qh
            for k in range(len(kids)):
                if k not in boxed:
                    rec["qlo" + ax][slots[k]], rec["qhi" + ax][slots[k]] = 255, 0
        recs.append(rec)
        w += 1
    return np.array(recs, bvh_check.NODE_DT), np.array(item_of_position, np.int64), T, np.array(slot_of_position, np.int64)


# ---------------------------------------------------------------------------------------------
# what a device tree must satisfy
# ---------------------------------------------------------------------------------------------
def check_tree(T, nodes, item_of_position, parts="abcdefg", boxes=None, what="tree"):
    """nodes: the records of ONE tree, its root first (child indices relative to it). item_of_position[p]: the API item at position p of
    the tree's item array. T: the restated Tree (order, topology, and the boxes the slots were dealt by); boxes: a Tree of the same
    topology holding the boxes the nodes must be quantised from now (after a refit), default T.
    -> dict(nodes, depth, cost, optimum, ratio, eps, height); raises AssertionError listing the problems, each tagged with its part."""
    B = boxes or T
    P, problems = T.P, []

    def bad(part, text):
        if part in parts and len(problems) < 40:
            problems.append(f"{what} [{part}] {text}")
    res = dict(nodes=0, depth=0, cost=0.0, optimum=T.optimum, ratio=0.0, eps=eps_of(T.height), height=T.height)
    if T.nleaves <= 1:
        if sorted(np.asarray(item_of_position).tolist()) != list(range(T.n)):
            bad("a", "the single leaf does not hold every item once")
        elif not np.array_equal(T.pos_of_item[item_of_position], np.arange(T.n)):
            bad("b", "the items of the single leaf are not in sorted order")
        assert not problems, "\n".join(problems)
        return res
    n_items = len(item_of_position)
    pos = T.pos_of_item[np.asarray(item_of_position, np.int64)] if n_items == T.n and n_items and int(np.max(item_of_position)) < T.n else None
    if pos is None or len(np.unique(pos)) != T.n:
        bad("a", f"the item array is not a permutation of the {T.n} items")
        assert not problems, "\n".join(problems)
        raise AssertionError(f"{what}: the item array is not a permutation of the items")
    # 1. walk: slots of every node, spans of sorted positions bottom-up
    info, order_seen, stack = {}, [], [(0, 1)]
    reached = np.zeros(n_items, np.int64)
    while stack:
        w, d = stack.pop()
        if w in info or w >= len(nodes) or d > 64:
            bad("a", f"node {w}: reached twice, out of range or deeper than 64"); continue
        n = nodes[w]
        slots, rank = [], 0
        for s in range(8):
            m = int(n["meta"][s])
            if m == 0:
                continue
            if (m & 0x1F) >= 24:
                if (m >> 5) != 1 or (m & 0x1F) != 24 + s or not (int(n["imask"]) >> s) & 1:
                    bad("f", f"node {w} slot {s}: internal meta {m:#x} against imask {int(n['imask']):#x}")
                child = int(n["childBase"]) + rank
                rank += 1
                slots.append((s, child, None, None)); stack.append((child, d + 1))
            else:
                cnt = {1: 1, 3: 2, 7: 3}.get(m >> 5)
                first = int(n["triBase"]) + (m & 0x1F)
                if (int(n["imask"]) >> s) & 1:
                    bad("f", f"node {w} slot {s}: a leaf slot flagged internal")
                if cnt is None or first + cnt > n_items:
                    bad("a", f"node {w} slot {s}: malformed leaf meta {m:#x} or items beyond the array"); continue
                reached[first:first + cnt] += 1
                slots.append((s, None, first, cnt))
        if bin(int(n["imask"])).count("1") != rank:
            bad("f", f"node {w}: imask {int(n['imask']):#x} names other slots than the {rank} internal metas")
        info[w] = (d, slots)
        order_seen.append(w)
        res["depth"] = max(res["depth"], d)
    res["nodes"] = len(order_seen)
    if not (reached == 1).all():
        bad("a", f"{int((reached != 1).sum())} positions of the item array are not reached exactly once")
    span = {}
    for w in reversed(order_seen):              # a child is discovered after its parent
        lo_p, hi_p, cnt_p = n_items, -1, 0
        for s, child, first, cnt in info[w][1]:
            if child is None:
                ps = pos[first:first + cnt]
                lo_p, hi_p, cnt_p = min(lo_p, int(ps.min())), max(hi_p, int(ps.max())), cnt_p + cnt
            elif child in span:
                lo_p, hi_p, cnt_p = min(lo_p, span[child][0]), max(hi_p, span[child][1]), cnt_p + span[child][2]
        span[w] = (lo_p, hi_p, cnt_p)
    L = P.leaf_size

    def ref_of_positions(a, b, cnt):
        """the binary node whose items are exactly the sorted positions a..b, or None"""
        if cnt != b - a + 1 or a % L or (b + 1) % L and b + 1 != T.n:
            return None
        return T.range_to_ref.get((a // L, b // L))
    # 2. top-down: every wide node against its binary node
    todo = [(0, 0)]
    while todo:
        w, root = todo.pop()
        if w not in info:
            continue
        n = nodes[w]
        depth, slots = info[w]
        kids = []                                # (first position, slot, ref, child, first, cnt)
        whole = True
        for s, child, first, cnt in slots:
            if child is None:
                ps = pos[first:first + cnt]
                a, b, c = int(ps.min()), int(ps.max()), cnt
                if not np.array_equal(ps, np.arange(a, a + cnt)):
                    bad("b" if sorted(ps.tolist()) == list(range(a, a + cnt)) else "a", f"node {w} slot {s}: its items stand at the sorted positions {ps.tolist()}")
            elif child in span:
                a, b, c = span[child]
            else:
                whole = False; continue
            ref = ref_of_positions(a, b, c)
            if ref is None:
                bad("a", f"node {w} slot {s}: the {c} items below it (sorted positions {a}..{b}) are no node of the binary tree"); whole = False; continue
            if child is None and T.items(ref) > P.max_leaf_items:
                bad("a", f"node {w} slot {s}: a leaf slot of {T.items(ref)} items")
            kids.append((a, s, ref, child, first, cnt))
        ra, rb = T.leaf_range(root)
        kids.sort()
        tiles = whole and kids and kids[0][0] == ra * L and all(kids[k][0] + T.items(kids[k][2]) == kids[k + 1][0] for k in range(len(kids) - 1)) \
            and kids[-1][0] + T.items(kids[-1][2]) == min((rb + 1) * L, T.n)
        if not tiles:
            bad("a", f"node {w}: its slots do not tile its binary node (leaves {ra}..{rb})")
            continue                              # what lies below cannot be named
        # b: leaf items contiguous from triBase in slot order
        run = 0
        for s, child, first, cnt in slots:
            if child is None:
                if first != int(n["triBase"]) + run:
                    bad("b", f"node {w} slot {s}: its items start at {first}, not at triBase + {run}")
                run += cnt
        # c
        res["cost"] += T.area(root) * P.cost_node + sum(T.leaf_cost(ref) if ref < 0 else T.area(ref) * T.items(ref) * P.cost_item
                                                        for _, _, ref, child, _, _ in kids if child is None)
        # f
        clo, chi = np.array([T.box(k[2])[0] for k in kids]), np.array([T.box(k[2])[1] for k in kids])
        want = slot_rule(*T.box(root), clo, chi)
        got = [k[1] for k in kids]
        if want != got:
            bad("f", f"node {w}: its children sit in the slots {got} from left to right, the rule deals them {want}")
        # d, e
        nlo, nhi = B.box(root)
        valid = bool((nlo <= nhi).all() and np.isfinite(nlo).all() and np.isfinite(nhi).all())
        if n["origin"].view(np.uint32).tolist() != (nlo if valid else np.zeros(3, f32)).view(np.uint32).tolist():
            bad("d", f"node {w}: origin {n['origin'].tolist()} is not the low corner {nlo.tolist()} of its binary node")
        occupied = {k[1] for k in kids}
        for s in range(8):
            if s not in occupied and (any(int(n["qlo" + a][s]) != 255 or int(n["qhi" + a][s]) != 0 for a in "xyz") or int(n["meta"][s])):
                bad("d", f"node {w} slot {s}: an empty slot not stored as [255, 0] with meta 0")
        for a in range(3):
            ax = "xyz"[a]
            e = int(n["exp"][a]) - 127
            boxed = [k for k in kids if valid and B.box(k[2])[0][a] <= B.box(k[2])[1][a]]
            far = max([B.box(k[2])[1][a] for k in boxed], default=nlo[a])          # (the node's own high side: its children tile it)
            if not (valid and float(nhi[a]) > float(nlo[a])):
                if e != -126:
                    bad("d", f"node {w} axis {ax}: exponent {e} on a zero extent, not -126")
            elif boxed:
                if not decode(n["origin"][a], 255, e) >= far:
                    bad("d", f"node {w} axis {ax}: at exponent {e} a child does not fit 0..255")
                elif e > -126 and fits(nlo[a], far, e - 1):
                    bad("d", f"node {w} axis {ax}: exponent {e}, but every child fits 0..255 at {e - 1} already")
            for k in kids:
                s = k[1]
                ql, qh = int(n["qlo" + ax][s]), int(n["qhi" + ax][s])
                lo_c, hi_c = B.box(k[2])[0][a], B.box(k[2])[1][a]
                if k not in boxed:
                    if (ql, qh) != (255, 0):
                        bad("d", f"node {w} slot {s} axis {ax}: a child without a box not stored as [255, 0]")
                    continue
                if ql > qh:
                    bad("e", f"node {w} slot {s} axis {ax}: stored as empty [{ql}, {qh}]"); continue
                dl, dh = float(decode(n["origin"][a], ql, e)), float(decode(n["origin"][a], qh, e))
                if dl > float(lo_c) or dh < float(hi_c):
                    bad("e", f"node {w} slot {s} axis {ax}: the padded box [{float(lo_c)!r}, {float(hi_c)!r}] sticks out of the decoded [{dl!r}, {dh!r}]")
                q = float(np.ldexp(1.0, e))
                if float(lo_c) - dl > q + U * max(abs(dl), abs(float(lo_c))) or dh - float(hi_c) > q + U * max(abs(dh), abs(float(hi_c))):
                    bad("e", f"node {w} slot {s} axis {ax}: decoded [{dl!r}, {dh!r}] lies more than a quantum 2^{e} outside [{float(lo_c)!r}, {float(hi_c)!r}]")
        for k in kids:
            if k[3] is not None:
                todo.append((k[3], k[2]))
    if res["optimum"] > 0:
        res["ratio"] = res["cost"] / res["optimum"] - 1.0
    if not any("[a]" in p for p in problems) and res["cost"] > res["optimum"] * (1.0 + res["eps"]):
        bad("c", f"cost {res['cost']!r} against the optimum {res['optimum']!r}: {res['ratio']:.3e} above it, eps = {res['eps']:.3e} ({res['ratio'] / res['eps']:.1f} eps)")
    assert not problems, "\n".join(problems)
    return res


def instance_boxes(inst, tris, root_bounds, nodes=None):
    """The items of the top level: instance_world_box of pt_bvh.hip, float32 with its operations one by one. The eight corners of the
    bottom level's root box pushed through objectToWorld, intersected with the box of the transformed vertices (meshes of at most 1024
    triangles, kExactBoxTriangles) or of the transformed child boxes two levels down as wide_child_box decodes them (larger meshes), moved
    outward by 2^-21 (|t_a| + sum_j |M_aj| (max |root box_j| + |W_j3|)). inst: INST_DT records in API order; tris, nodes: every packet and node of the
    copy; root_bounds(instance) -> (lo, hi) of its bottom level's root. -> lo, hi [n, 3] float32, unpadded."""
    n = len(inst)
    lo, hi = np.full((n, 3), np.inf, f32), np.full((n, 3), -np.inf, f32)

    def slot_box(nd, s):
        e = nd["exp"].astype(np.int64) - 127
        ql = np.array([nd["qlox"][s], nd["qloy"][s], nd["qloz"][s]]); qh = np.array([nd["qhix"][s], nd["qhiy"][s], nd["qhiz"][s]])
        if (ql > qh).any():
            return None
        return np.array([decode(nd["origin"][a], ql[a], e[a]) for a in range(3)], f32), np.array([decode(nd["origin"][a], qh[a], e[a]) for a in range(3)], f32)
    with np.errstate(all="ignore"):
        for i in range(n):
            it = inst[i]
            blo, bhi = root_bounds(i)
            if not blo[0] <= bhi[0]:
                continue                                                           # an empty bottom level: the box stays inverted
            tc = int(it["triCount"])
            M, Wm = it["objectToWorld"].astype(f32).reshape(3, 4), it["worldToObject"].astype(f32).reshape(3, 4)

            def xf(p):
                return (((M[:, 0] * p[:, 0:1]).astype(f32) + (M[:, 1] * p[:, 1:2]).astype(f32)).astype(f32) + (M[:, 2] * p[:, 2:3]).astype(f32)).astype(f32) + M[:, 3]

            def corners(l, h):
                return xf(np.array([[(h if c & 1 else l)[0], (h if c & 2 else l)[1], (h if c & 4 else l)[2]] for c in range(8)], f32)).astype(f32)
            wc = corners(blo, bhi)
            l, h = wc.min(0), wc.max(0)
            if tc <= 1024:
                t = tris[int(it["triBase"]):int(it["triBase"]) + tc]
                wv = xf(np.concatenate([t["v0"], t["v1"], t["v2"]]).astype(f32)).astype(f32)
                l, h = np.maximum(l, wv.min(0)), np.minimum(h, wv.max(0))
            else:
                assert nodes is not None
                nb = int(it["nodeBase"])
                root = nodes[nb]
                boxes, rank = [], 0
                for s in range(8):
                    c = slot_box(root, s)
                    internal = (int(root["imask"]) >> s) & 1
                    if internal:
                        child = nodes[nb + int(root["childBase"]) + rank]
                        rank += 1
                    if c is None:
                        continue
                    if not internal:
                        boxes.append(corners(*c)); continue
                    for t_ in range(8):
                        g = slot_box(child, t_)
                        if g is None:
                            continue
                        gl, gh = np.maximum(g[0], c[0]), np.minimum(g[1], c[1])
                        if (gl <= gh).all():
                            boxes.append(corners(gl, gh))
                tl, th = (np.concatenate(boxes).min(0), np.concatenate(boxes).max(0)) if boxes else (np.full(3, np.inf, f32), np.full(3, -np.inf, f32))
                l, h = np.maximum(l, tl), np.minimum(h, th)
                if not (l <= h).all():
                    l, h = np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
            if l[0] <= h[0]:
                for a in range(3):
                    s = np.abs(M[a, 3])
                    for j in range(3):
                        w = np.abs(Wm[j, 3])
                        s = f32(s + f32(np.abs(M[a, j]) * f32(np.maximum(np.abs(blo[j]), np.abs(bhi[j])) + (w if w < np.inf else f32(0)))))
                    e = f32(s * f32(4.76837158e-7))
                    if e < np.inf:
                        l[a], h[a] = f32(l[a] - e), f32(h[a] + e)
            lo[i], hi[i] = l, h
    return lo, hi


def check(layout, buf, blas_params, tlas_params, parts="abcdefg", accel=None, built=None):
    """Every distinct bottom level and the top level of a downloaded traversal copy. blas_params(triangle count) -> Params.
    accel: accel_stats() of the context, for part g. built: the result of check() right after the build; then the order, the topology and
    the slot rule are taken from it (a refit keeps them) and only the boxes from the vertices as they are now, and part c is not asked.
    -> dict(trees={key: (Tree, result of check_tree)}, ratio, ratio_of, eps_of_worst, large)"""
    inst, nodes, tris, order = bvh_check.split(layout, buf)
    out = dict(trees={}, ratio=0.0, ratio_of=None, large=0)
    if built:
        parts = parts.replace("c", "")
    problems = []
    node_bytes, blas_depth = (len(inst) + 1) * 80, 0
    roots = {}
    for i, it in enumerate(inst):
        key = (int(it["nodeBase"]), int(it["triBase"]), int(it["triCount"]))
        if key not in out["trees"]:
            nb, tb, tc = key
            t = tris[tb:tb + tc]
            lo, hi, api = triangle_boxes(t)
            if built:
                T = built["trees"][key][0]
                B = Tree.__new__(Tree); B.__dict__.update(T.__dict__); B.rebox(lo, hi)
            else:
                T = B = Tree(lo, hi, blas_params(tc))
            try:
                r = check_tree(T, nodes[nb:], api, parts, boxes=B, what=f"bottom level of instance {i} ({tc} triangles)")
            except AssertionError as e:
                problems.append(str(e)); r = None
            out["trees"][key] = (T, r, B)
            if r:
                node_bytes += max(r["nodes"], 1) * 80; blas_depth = max(blas_depth, r["depth"])
                if r["ratio"] > out["ratio"]:
                    out["ratio"], out["ratio_of"] = r["ratio"], f"bottom level, {tc} triangles, H = {r['height']}"
        roots[i] = out["trees"][key][2].root_bounds()
    if len(inst):
        lo, hi = instance_boxes(inst, tris, lambda i: roots[i], nodes)
        plo, phi = pad_boxes(lo, hi)
        same = (plo.view(np.uint32) == inst["boxLo"].view(np.uint32)).all(1) & (phi.view(np.uint32) == inst["boxHi"].view(np.uint32)).all(1)
        if not same.all() and "a" in parts:
            i = int(np.nonzero(~same)[0][0])
            problems.append(f"top level [a] {int((~same).sum())} instance records do not hold pad_box of the restated world box, first {i}: "
                            f"{inst['boxLo'][i].tolist()} {inst['boxHi'][i].tolist()} against {plo[i].tolist()} {phi[i].tolist()}")
        T = Tree(lo, hi, tlas_params)                # the top level is rebuilt, never refitted: always restated from the boxes as they are
        out["large"] = int(T.large.sum())
        try:
            r = check_tree(T, nodes, order.astype(np.int64), parts, what=f"top level ({len(inst)} instances)")
        except AssertionError as e:
            problems.append(str(e)); r = None
        out["tlas"] = (T, r)
        if r and not built and r["ratio"] > out["ratio"]:
            out["ratio"], out["ratio_of"] = r["ratio"], f"top level, {len(inst)} instances, H = {r['height']}"
        if accel is not None and "g" in parts and r and not problems:
            if int(accel.NodeBytes) != node_bytes:
                problems.append(f"[g] accel_stats: {int(accel.NodeBytes)} node bytes, the walked trees have {node_bytes}")
            if int(accel.MaxBottomLevelDepth) != blas_depth or int(accel.TopLevelDepth) != r["depth"]:
                problems.append(f"[g] accel_stats: depths {int(accel.MaxBottomLevelDepth)} / {int(accel.TopLevelDepth)}, walked {blas_depth} / {r['depth']}")
    assert not problems, "\n".join(problems)
    return out
