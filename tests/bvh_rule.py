"""The tree of a leaf set, stated a third time (TEST INFRASTRUCTURE; DESIGN.md section 4, rules B1-B12).

csrc/lbvh.hip, the host's TLAS builder and oracle/oracle_bvh.c all follow Karras' construction, written from one "Geometry spec" by one hand.  This
module states what that construction has to produce from the MEANING of a linear BVH, in numpy only; it imports nothing from oracle/ and nothing
from the library, and it never runs Karras' searches.  No Python loop runs over leaves or nodes: the loops here run over the bits of a key, over the
levels of the key trie (at most 62) and over the levels of the tree (at most 62 too: a radix tree over 62-bit keys is no deeper).

B1  Leaf box: min and max of the three corners (exact: a min or max picks one of its arguments).  -0 orders below +0, as v_min_f32 / v_max_f32 and
    IEEE 754-2019 minimum / maximum have it; the rule takes every min and max on the order-preserving integer image of a float32, so it is definite.
B2  Scene box = min / max over all leaf boxes.  Key of a leaf, float32 operation by operation:
        c = (mn + mx) * 0.5        ext = bmax - bmin        scale = ext > 0 ? 1024 / ext : 0
        q = clamp(trunc((c - bmin) * scale), 0, 1023)       code = interleave(q), x in bit 0, y in bit 1, z in bit 2 of every triple
    Why the float32 restatement is exact: every one of these expressions is a chain of single IEEE 754 binary32 operations (add, subtract, multiply,
    divide), each correctly rounded, and numpy evaluates a float32 array expression one such operation at a time.  The one licence a compiler has to
    change a result, contracting a multiply and a DEPENDENT ADD into a fused multiply-add, needs a product that feeds a sum; here every product is
    the last operation of its expression ((a + b) * 0.5, (c - bmin) * scale: a sum feeds the product, never the reverse), so no fused multiply-add
    can arise whatever -ffp-contract says, and any conforming implementation gives these bits.
B3  Order: ascending by the 62-bit key  code << 32 | leaf  (unique), i.e. a stable sort by code.
B4  Tree, by definition and not by search.  Let h[g] be the highest bit in which sorted keys g and g + 1 differ.  Inside any range of sorted keys
    that share a prefix, the largest h occurs exactly once (it is where the first bit below the prefix turns from 0 to 1), so the radix tree is the
    Cartesian tree of h: the split g owns the maximal range [lo, hi] in which h[g] is the largest, lo - 1 = the nearest pair to the left with a
    larger h, hi = the nearest pair to the right with a larger h (0 and n - 1 where there is none).  Of those two bounding pairs the one with the
    SMALLER h is the parent's split.  A node that is the left part of its parent ends at the parent's split and is called by its last leaf, hi; a
    right part is called by its first leaf, lo; the root is node 0.  So node i covers the maximal range with i in {lo, hi}; `pad` is the other end.
    left = leaf lo if lo == g else node g;  right = leaf g + 1 if hi == g + 1 else node g + 1.  parent and leafParent follow.
B5  Boxes: the left / right box of a node is the min / max of the sorted leaf boxes over [lo, g] / [g + 1, hi] (np.minimum.reduceat over those
    index pairs: no link of the tree is followed).  Exact for the same reason as B1.
B6  Header: box of all leaves, count = n, depth = inner nodes on the longest root-to-leaf path.
B7  One leaf: node 0 = {left = leaf 0, right = none, parent = none, pad = 0, right box +inf / -inf}, depth 1.
B8  Triangle record s: the three corners and prim = sortedIndex[s], pad words 0.
B9  Refit: keys, order and every link as the first build left them; boxes, header box and triangle records from the moved leaves over the old ranges.
B10 TLAS: the leaves are instances; everything above the leaves is held exactly (B2-B7) from the leaf boxes as they stand in the tree's leaf slots.
B11 TLAS leaf box: the box of the mesh box's eight corners p through objectToWorld (row vectors: w_k = sum_j p_j m_jk + t_k), computed in float32 in
    an order this rule does not assume.  Each product carries one rounding, (1 + d), |d| <= u = 2^-24 (none if fused); each of the three additions
    carries one more for every term that has entered the sum by then.  A term passes through at most 4 roundings whatever the order of the
    additions and whether or not products are fused, so |fl(w_k) - w_k| <= ((1 + u)^4 - 1) * (sum_j |p_j m_jk| + |t_k|) = gamma_4 * S_k, plus one
    smallest subnormal per operation for underflow.  min and max over the corners move by no more than their arguments do, so each stored bound
    lies within the largest gamma_4 * S_k of the eight corners of the float64 bound.  Nothing of this is measured.
B12 Out of scope: NaN or infinite positions, three group levels of the large fit (more than 8.3 M leaves), traversal (ray_rule.py, oracle parity).

Time: the check of the 524289-leaf oracle tree (scattered: the rule's own tree, then the comparison field by field) takes 1.3 to 1.5 s on the CPU it was
written on, all but 0.2 s of it the rule's tree; tests/test_bvh_rule.py fails above 10 s."""
import numpy as np

LEAF = 0x80000000
NONE = 0xFFFFFFFF
NODE_DTYPE = np.dtype([("lmin", "<f4", 3), ("lmax", "<f4", 3), ("rmin", "<f4", 3), ("rmax", "<f4", 3), ("left", "<u4"), ("right", "<u4"), ("parent", "<u4"), ("pad", "<u4")])
TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("prim", "<u4"), ("v1", "<f4", 3), ("pad1", "<u4"), ("v2", "<f4", 3), ("pad2", "<u4")])
assert NODE_DTYPE.itemsize == 64 and TRI_DTYPE.itemsize == 48

MUTATIONS = ("key_from_box_minimum", "quantised_by_1023", "y_z_exchanged")         # wrong readings of B2 the rule can build a whole tree from
U = 2.0 ** -24
GAMMA4 = (1.0 + U) ** 4 - 1.0


def _ordered(f):
    """float32 -> uint32 whose integer order is the order of the floats, -0 below +0."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(LEAF), ~u, u | np.uint32(LEAF))


def _floats(o):
    o = np.ascontiguousarray(o, dtype=np.uint32)
    return np.where(o & np.uint32(LEAF), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def leaf_boxes(positions, indices):
    """B1 -> (mn [n, 3], mx [n, 3], corners [n, 3, 3])"""
    p = np.ascontiguousarray(positions, dtype=np.float32)[:, :3]
    tri = p[np.asarray(indices, dtype=np.int64)].reshape(-1, 3, 3)
    o = _ordered(tri)
    return _floats(o.min(axis=1)), _floats(o.max(axis=1)), tri


def _interleave(q, mutate=None):
    shift = (0, 2, 1) if mutate == "y_z_exchanged" else (0, 1, 2)
    code = np.zeros(len(q), dtype=np.uint32)
    for b in range(10):                                                            # bits of a coordinate
        for k in range(3):
            code |= ((q[:, k] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + shift[k])
    return code


def keys(mn, mx, mutate=None):
    """B2 -> (bmin, bmax, code [n] in leaf order)"""
    assert mutate is None or mutate in MUTATIONS, mutate
    f32 = np.float32
    bmin, bmax = _floats(_ordered(mn).min(axis=0)), _floats(_ordered(mx).max(axis=0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ext = bmax - bmin
        scale = np.where(ext > f32(0.0), f32(1023.0 if mutate == "quantised_by_1023" else 1024.0) / ext, f32(0.0)).astype(f32)
        c = mn if mutate == "key_from_box_minimum" else (mn + mx) * f32(0.5)
        f = (c - bmin) * scale
    assert f.dtype == np.float32 and scale.dtype == np.float32
    q = np.clip(np.trunc(f), 0.0, 1023.0).astype(np.uint32)
    return bmin, bmax, _interleave(q, mutate)


def _highest_bit(x):
    x = x.copy(); h = np.zeros(len(x), dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(s)) != 0
        h += s * m
        x = np.where(m, x >> np.uint64(s), x)
    return h


def topology(code, order):
    """B4 from the sorted keys -> dict of per-node arrays (left, right, parent, pad, lo, split, hi), leafParent and depth.  n >= 2."""
    n = len(code)
    key = (code.astype(np.uint64) << np.uint64(32)) | order.astype(np.uint64)
    assert np.all(key[1:] > key[:-1]), "keys are not sorted ascending"
    m = n - 1
    h = _highest_bit(key[:-1] ^ key[1:])
    idx = np.arange(m, dtype=np.int64)
    before = np.full(m, -1, dtype=np.int64); after = np.full(m, m, dtype=np.int64)
    for b in np.unique(h):                                                         # levels of the key trie
        sel = h == b; larger = h > b
        before[sel] = np.maximum.accumulate(np.where(larger, idx, -1))[sel]
        after[sel] = np.minimum.accumulate(np.where(larger, idx, m)[::-1])[::-1][sel]
    lo, hi = before + 1, after
    h_before = np.where(before >= 0, h[np.maximum(before, 0)], 64); h_after = np.where(after < m, h[np.minimum(after, m - 1)], 64)
    root = (before < 0) & (after >= m)
    assert root.sum() == 1
    is_left = h_after < h_before                                                   # the parent's split is the bounding pair with the smaller h
    name = np.where(root, 0, np.where(is_left, hi, lo))
    assert np.array_equal(np.sort(name), idx), "node names are not a permutation"
    parent_split = np.where(is_left, after, before)
    t = dict(lo=np.empty(m, np.int64), hi=np.empty(m, np.int64), split=np.empty(m, np.int64))
    t["lo"][name] = lo; t["hi"][name] = hi; t["split"][name] = idx
    left = np.where(lo == idx, idx | LEAF, idx).astype(np.uint32); right = np.where(hi == idx + 1, (idx + 1) | LEAF, idx + 1).astype(np.uint32)
    parent = np.where(root, NONE, name[np.clip(parent_split, 0, m - 1)]).astype(np.uint32)
    for f, v in (("left", left), ("right", right), ("parent", parent), ("pad", (lo + hi - name).astype(np.uint32))):
        t[f] = np.empty(m, np.uint32); t[f][name] = v
    leaf_parent = np.empty(n, dtype=np.uint32)
    leaf_parent[idx[lo == idx]] = name[lo == idx]; leaf_parent[idx[hi == idx + 1] + 1] = name[hi == idx + 1]
    depth = np.zeros(m, dtype=np.int64); depth[0] = 1
    safe = np.where(t["parent"] == NONE, 0, t["parent"]).astype(np.int64)
    for _ in range(64):                                                            # levels of the tree
        todo = (depth == 0) & (depth[safe] > 0)
        if not todo.any():
            break
        depth[todo] = depth[safe[todo]] + 1
    assert np.all(depth > 0)
    t["leafParent"] = leaf_parent; t["depth"] = int(depth.max())
    return t


def _range_boxes(mn_o, mxi_o, start, end):
    """min over [start, end) of the six columns (ordered mins, inverted ordered maxes) by one reduceat; segments sorted by start, so that what
    reduceat reduces between two segments is disjoint from one gap to the next (O(n) in all)."""
    six = np.concatenate([mn_o, mxi_o], axis=1)
    six = np.concatenate([six, six[-1:]], axis=0)
    by = np.argsort(start, kind="stable")
    pairs = np.stack([start[by], end[by]], axis=1).ravel()
    out = np.empty((len(start), 6), dtype=np.uint32)
    out[by] = np.minimum.reduceat(six, pairs, axis=0)[::2]
    return _floats(out[:, :3]), _floats(~out[:, 3:])


def build(mn, mx, mutate=None, order=None, code=None):
    """B2-B7 from leaf boxes in leaf order.  With order / code given (B9) the keys are those and only the boxes are new."""
    n = len(mn)
    bmin, bmax, c = keys(mn, mx, mutate)
    if order is None:
        order = np.argsort((c.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64), kind="stable").astype(np.uint32)
        code = c[order]
    smn, smx = mn[order], mx[order]
    nodes = np.zeros(max(n - 1, 1), dtype=NODE_DTYPE)
    if n == 1:
        nodes["left"], nodes["right"], nodes["parent"], nodes["pad"] = LEAF, NONE, NONE, 0
        nodes["lmin"], nodes["lmax"], nodes["rmin"], nodes["rmax"] = smn, smx, np.inf, -np.inf
        t = dict(leafParent=np.zeros(1, np.uint32), depth=1, lo=np.zeros(1, np.int64), hi=np.zeros(1, np.int64), split=np.zeros(1, np.int64))
    else:
        t = topology(code, order)
        for f in ("left", "right", "parent", "pad"):
            nodes[f] = t[f]
        mn_o, mxi_o = _ordered(smn), ~_ordered(smx)
        nodes["lmin"], nodes["lmax"] = _range_boxes(mn_o, mxi_o, t["lo"], t["split"] + 1)
        nodes["rmin"], nodes["rmax"] = _range_boxes(mn_o, mxi_o, t["split"] + 1, t["hi"] + 1)
    return dict(count=n, morton=code, sortedIndex=order, nodes=nodes, bmin=bmin, bmax=bmax, depth=t["depth"], leafParent=t["leafParent"],
                lo=t["lo"], hi=t["hi"], split=t["split"], leafMin=smn, leafMax=smx)


def _triangles(corners, order):
    tris = np.zeros(len(order), dtype=TRI_DTYPE)
    c = corners[order]
    tris["v0"], tris["v1"], tris["v2"], tris["prim"] = c[:, 0], c[:, 1], c[:, 2], order
    return tris


def mesh_tree(positions, indices, mutate=None):
    mn, mx, corners = leaf_boxes(positions, indices)
    t = build(mn, mx, mutate)
    t["tris"] = _triangles(corners, t["sortedIndex"])
    return t


def refit_tree(first, positions, indices):
    """B9: `first` is the rule's tree of the first build."""
    mn, mx, corners = leaf_boxes(positions, indices)
    assert len(mn) == first["count"]
    t = build(mn, mx, order=first["sortedIndex"], code=first["morton"])
    t["tris"] = _triangles(corners, t["sortedIndex"])
    return t


def tree_of(morton, sorted_index, nodes, header=None, tris=None, bmin=None, bmax=None, count=None, depth=None):
    """A tree as read back (header: the 8 words of BlasHeader = bmin[3], count, bmax[3], depth) or as the oracle hands it out (no depth)."""
    if header is not None:
        w = np.ascontiguousarray(header).view(np.uint32)
        bmin, count, bmax, depth = w[0:3].view(np.float32), int(w[3]), w[4:7].view(np.float32), int(w[7])
    return dict(morton=np.asarray(morton), sortedIndex=np.asarray(sorted_index), nodes=nodes, tris=tris, bmin=np.asarray(bmin, dtype=np.float32),
                bmax=np.asarray(bmax, dtype=np.float32), count=count, depth=depth)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _differ(findings, label, got, want):
    got, want = _bits(got), _bits(want)
    if got.shape != want.shape:
        findings.append("%s: %d entries, the rule has %d" % (label, len(got), len(want))); return
    bad = got != want
    if bad.any():
        k = int(np.argmax(bad))
        findings.append("%s[%d]: %s, the rule has %s (%d entries in all)" % (label, k, got[k], want[k], int(bad.sum())))


def compare(got, want, depth="rule", prefix=""):
    """Findings, field by field: `got` from tree_of, `want` from the rule.  depth: "rule", a number the header must hold, or None (not held)."""
    out = []
    if got["count"] is not None and got["count"] != want["count"]:
        out.append("header.count: %s, the rule has %s" % (got["count"], want["count"]))
    _differ(out, "morton", got["morton"], want["morton"])
    _differ(out, "sortedIndex", got["sortedIndex"], want["sortedIndex"])
    if len(got["nodes"]) != len(want["nodes"]):
        out.append("nodes: %d, the rule has %d" % (len(got["nodes"]), len(want["nodes"])))
    else:
        for f in ("left", "right", "parent", "pad", "lmin", "lmax", "rmin", "rmax"):
            g, w = _bits(got["nodes"][f]), _bits(want["nodes"][f])
            bad = g != w
            if bad.ndim > 1:
                bad = bad.any(axis=1)
            if bad.any():
                k = int(np.argmax(bad))
                out.append("node %d.%s: %s, the rule has %s (%d nodes in all)" % (k, f, got["nodes"][f][k], want["nodes"][f][k], int(bad.sum())))
    if got.get("tris") is not None and want.get("tris") is not None:
        if len(got["tris"]) < want["count"]:
            out.append("triangles: %d records, the rule has %d" % (len(got["tris"]), want["count"]))
        else:
            for f in ("v0", "v1", "v2", "prim", "pad1", "pad2"):
                g, w = _bits(got["tris"][f][:want["count"]]), _bits(want["tris"][f])
                bad = g != w
                if bad.ndim > 1:
                    bad = bad.any(axis=1)
                if bad.any():
                    k = int(np.argmax(bad))
                    out.append("triangle %d.%s: %s, the rule has %s (%d records in all)" % (k, f, got["tris"][f][k], want["tris"][f][k], int(bad.sum())))
    for f in ("bmin", "bmax"):
        if not np.array_equal(_bits(got[f]), _bits(want[f])):
            out.append("header.%s: %s, the rule has %s" % (f, got[f], want[f]))
    if depth is not None:
        d = want["depth"] if depth == "rule" else depth
        if got["depth"] != d:
            out.append("header.depth: %s, %s" % (got["depth"], "the rule has %d" % d if depth == "rule" else "a tree of the multi-kernel path holds %d" % d))
    return [prefix + s for s in out]


def check_mesh(got, positions, indices, depth="rule"):
    return compare(got, mesh_tree(positions, indices), depth)


def check_refit(got, first, positions, indices, depth="rule"):
    return compare(got, refit_tree(first, positions, indices), depth, prefix="refit: ")


def leaf_slots(got):
    """The leaf boxes as they stand in the tree's leaf-child slots -> (mn, mx) in SORTED order, findings."""
    n = len(got["sortedIndex"]); nodes = got["nodes"]
    mn = np.full((n, 3), np.nan, dtype=np.float32); mx = np.full((n, 3), np.nan, dtype=np.float32); seen = np.zeros(n, dtype=np.int64)
    for side, lo_f, hi_f in (("left", "lmin", "lmax"), ("right", "rmin", "rmax")):
        c = nodes[side]
        is_leaf = ((c & np.uint32(LEAF)) != 0) & (c != np.uint32(NONE))
        s = (c[is_leaf] & np.uint32(0x7FFFFFFF)).astype(np.int64)
        if (s >= n).any():
            return mn, mx, ["node %d.%s: leaf %d of %d" % (int(np.flatnonzero(is_leaf)[np.argmax(s >= n)]), side, int(s.max()), n)]
        np.add.at(seen, s, 1)
        mn[s] = nodes[lo_f][is_leaf]; mx[s] = nodes[hi_f][is_leaf]
    bad = seen != 1
    return mn, mx, (["leaf %d: the child of %d nodes (%d leaves in all)" % (int(np.argmax(bad)), int(seen[np.argmax(bad)]), int(bad.sum()))] if bad.any() else [])


def instance_boxes(mesh_min, mesh_max, transforms):
    """B11 in float64 -> (mn, mx, bound), each [m, 3] in instance order."""
    lo, hi = np.asarray(mesh_min, dtype=np.float64), np.asarray(mesh_max, dtype=np.float64)
    m = np.asarray(transforms, dtype=np.float64)                                   # [m, 4, 4], row vectors
    pick = np.array([[(c >> k) & 1 for k in range(3)] for c in range(8)], dtype=bool)          # [8, 3]
    p = np.where(pick[None], hi[:, None, :], lo[:, None, :])                       # [m, 8, 3]
    terms = p[:, :, :, None] * m[:, None, :3, :3]                                  # [m, 8, j, k]
    w = terms.sum(axis=2) + m[:, None, 3, :3]
    s = np.abs(terms).sum(axis=2) + np.abs(m[:, None, 3, :3])
    bound = (GAMMA4 * s).max(axis=1) + 7 * 2.0 ** -149
    return w.min(axis=1), w.max(axis=1), bound


def check_tlas(got, mesh_min, mesh_max, transforms, depth="rule"):
    """B10 + B11 -> (findings, largest |stored - float64| / bound over all leaf boxes)."""
    order = np.asarray(got["sortedIndex"]).astype(np.int64); n = len(order)
    if not np.array_equal(np.sort(order), np.arange(n)):
        return ["sortedIndex: not a permutation of the %d instances" % n], 0.0
    smn, smx, out = leaf_slots(got)
    if out:
        return out, 0.0
    mn = np.empty_like(smn); mx = np.empty_like(smx); mn[order] = smn; mx[order] = smx
    out = compare(got, build(mn, mx), depth)
    wmn, wmx, bound = instance_boxes(mesh_min, mesh_max, transforms)
    ratio = np.maximum(np.abs(mn.astype(np.float64) - wmn), np.abs(mx.astype(np.float64) - wmx)) / bound
    bad = ~(ratio <= 1.0)
    if bad.any():
        i, k = np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape)
        out.append("leaf box of instance %d, axis %d: [%.9g, %.9g] against [%.17g, %.17g] in float64, bound %.3g (%d bounds in all)" % (i, k, mn[i, k], mx[i, k], wmn[i, k], wmx[i, k], bound[i, k], int(bad.sum())))
    return out, float(np.nanmax(ratio))
