"""Device builder 2 (csrc/bvh_ploc.hip between the leaves and the emit step of csrc/bvh_device.hip) restated in numpy and
Python integers, with builder 1's hierarchy for the case in which builder 2 gives up.

  keys / order  as tests/test_gpu_lbvh.py states them: centroid 0.5f * (lo + hi); bounds = min / max of the centroids; per
                axis the cell trunc(clamp((c - lo) / max(hi - lo, 1e-30f) * 2097152, 0, 2097151)) in float32; the three
                cells interleaved x, y, z from the top bit; a stable sort.
  leaves        L = (n + 1) // 2 leaves of two consecutive sorted primitives (the last of an odd n holds one); a leaf's box
                is the min / max of its primitives' boxes, its key the key of its first primitive.
  clustering    the live clusters in slots 0 .. m-1, at first the leaves in order, each with a box, a code (~leaf, or the
                node index of a merged cluster) and an inner depth (0 for a leaf).  One round: nn[i] = the j != i in
                [max(0, i - 8), min(m - 1, i + 8)] with the least d(i, j), the lowest j on ties; d = dx*dy + dy*dz + dz*dx in
                float32 (each product and sum rounded, left to right) over the union box min / max.  Slots with
                nn[nn[i]] == i and i < nn[i] merge: child0 = slot i's code, child1 = slot nn[i]'s, box = union, depth =
                max + 1; the merged cluster stays in slot i, slot nn[i] dies.  A round of k merges numbers them, in slot
                order, next - k .. next - 1 and sets next -= k (next = L - 1 at first), so the root is node 0.  The live
                slots are compacted in order.  At most 95 rounds: with more than one cluster left after them the tree is
                builder 1's (fell_back).
  builder 1     a range [a, b] of leaves (keys made unique as key << 32 | leaf index) splits after the last leaf that
                agrees with leaf a on the highest bit in which a and b differ; Karras' numbering: the root 0, a left child
                the LAST leaf of its range, a right child the FIRST of its.
  cost          the emit kernel's formula in float64: per node 1.2 * area(own box), per leaf child count * area(leaf box),
                over the root's area, area = dx*dy + dy*dz + dz*dx.
"""
import numpy as np

F32 = np.float32
RADIUS = 8
MAX_ROUNDS = 95
COST_TRAVERSE, COST_INTERSECT = 1.2, 1.0           # csrc/bvh_builder.h: BvhOptions


def morton_keys(lo, hi):
    c = F32(0.5) * (lo + hi)
    assert c.dtype == F32
    blo, bhi = c.min(0), c.max(0)
    ext = np.maximum(bhi - blo, F32(1e-30))
    raw = (c - blo) / ext * F32(2097152.0)
    assert raw.dtype == F32
    cell = np.minimum(np.maximum(raw, F32(0.0)), F32(2097151.0)).astype(np.uint64)
    keys = np.zeros(len(c), np.uint64)
    for bit in range(21):
        for a in range(3):
            keys |= ((cell[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + 2 - a)
    return keys


def sorted_leaves(lo, hi):
    """(order [n], leaf_lo [L, 3], leaf_hi [L, 3], leaf_keys [L])"""
    n = len(lo)
    keys = morton_keys(lo, hi)
    order = np.argsort(keys, kind="stable")
    slo, shi = lo[order], hi[order]
    leaf_lo, leaf_hi = slo[0::2].copy(), shi[0::2].copy()
    second = np.arange(1, n, 2)
    leaf_lo[:len(second)] = np.minimum(leaf_lo[:len(second)], slo[second])
    leaf_hi[:len(second)] = np.maximum(leaf_hi[:len(second)], shi[second])
    return order, leaf_lo, leaf_hi, np.ascontiguousarray(keys[order][0::2])


def half_area32(lo, hi):
    d = hi - lo
    assert d.dtype == F32
    out = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
    assert out.dtype == F32
    return out


def half_area64(lo, hi):
    d = hi.astype(np.float64) - lo.astype(np.float64)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def nearest(lo, hi):
    """nn [m] of one round over the cluster boxes."""
    m = len(lo)
    dist = np.full((m, 2 * RADIUS), np.inf, F32)
    other = np.full((m, 2 * RADIUS), -1, np.int64)
    for col, off in enumerate(list(range(-RADIUS, 0)) + list(range(1, RADIUS + 1))):          # columns in ascending j
        i = np.arange(max(0, -off), min(m, m - off))
        if len(i):
            j = i + off
            dist[i, col] = half_area32(np.minimum(lo[i], lo[j]), np.maximum(hi[i], hi[j]))
            other[i, col] = j
    assert np.isfinite(dist[other >= 0]).all()
    return other[np.arange(m), np.argmin(dist, 1)]                                            # (argmin: the first minimum)


def ploc_hierarchy(leaf_lo, leaf_hi):
    """(child [L-1, 2] codes, node_lo, node_hi [L-1, 3], root depth, rounds) or None when clusters are left after the
    last round."""
    L = len(leaf_lo)
    lo, hi = leaf_lo.copy(), leaf_hi.copy()
    code, depth = ~np.arange(L, dtype=np.int64), np.zeros(L, np.int64)
    child = np.zeros((L - 1, 2), np.int64)
    node_lo, node_hi = np.zeros((L - 1, 3), F32), np.zeros((L - 1, 3), F32)
    nxt, rounds = L - 1, 0
    while len(code) > 1:
        if rounds == MAX_ROUNDS:
            return None
        m = len(code)
        nn = nearest(lo, hi)
        slot = np.arange(m)
        first = np.flatnonzero((nn[nn] == slot) & (slot < nn))
        second = nn[first]
        k = len(first)
        assert k >= 1
        node = nxt - k + np.arange(k)
        child[node, 0], child[node, 1] = code[first], code[second]
        node_lo[node], node_hi[node] = np.minimum(lo[first], lo[second]), np.maximum(hi[first], hi[second])
        lo[first], hi[first] = node_lo[node], node_hi[node]
        depth[first] = np.maximum(depth[first], depth[second]) + 1
        code[first] = node
        live = np.ones(m, bool)
        live[second] = False
        lo, hi, code, depth = lo[live], hi[live], code[live], depth[live]
        nxt -= k
        rounds += 1
    assert nxt == 0 and code[0] == 0
    return child, node_lo, node_hi, int(depth[0]), rounds


def lbvh_hierarchy(leaf_lo, leaf_hi, leaf_keys):
    """Builder 1: (child [L-1, 2] codes, node_lo, node_hi, root depth)."""
    L = len(leaf_keys)
    k = [(int(v) << 32) | j for j, v in enumerate(leaf_keys)]
    child = np.zeros((L - 1, 2), np.int64)
    ranges = np.zeros((L - 1, 2), np.int64)
    inner = np.zeros(L - 1, np.int64)                  # inner nodes from the root down to this one
    visit = []
    stack = [(0, 0, L - 1, 1)]
    while stack:
        node, a, b, d = stack.pop()
        visit.append(node)
        ranges[node], inner[node] = (a, b), d
        p = (k[a] ^ k[b]).bit_length() - 1
        bound = ((k[a] >> p) + 1) << p                 # the first key that no longer agrees with leaf a on bit p
        lo_, hi_ = a, b                                # the last leaf in [a, b] with a key below bound
        while lo_ < hi_:
            mid = (lo_ + hi_ + 1) // 2
            if k[mid] < bound:
                lo_ = mid
            else:
                hi_ = mid - 1
        g = lo_
        assert a <= g < b
        if a == g:
            child[node, 0] = ~g
        else:
            child[node, 0] = g
            stack.append((g, a, g, d + 1))
        if g + 1 == b:
            child[node, 1] = ~b
        else:
            child[node, 1] = g + 1
            stack.append((g + 1, g + 1, b, d + 1))
    node_lo, node_hi = np.zeros((L - 1, 3), F32), np.zeros((L - 1, 3), F32)
    for node in range(L - 1):
        a, b = ranges[node]
        node_lo[node], node_hi[node] = leaf_lo[a:b + 1].min(0), leaf_hi[a:b + 1].max(0)
    return child, node_lo, node_hi, int(inner.max())


def child_boxes(t):
    """([L-1, 2, 3] lo, hi): the boxes of every node's two children."""
    c = t["child"]
    leaf = c < 0
    at_leaf, at_node = np.where(leaf, ~c, 0), np.where(leaf, 0, c)
    lo = np.where(leaf[..., None], t["leaf_lo"][at_leaf], t["node_lo"][at_node])
    hi = np.where(leaf[..., None], t["leaf_hi"][at_leaf], t["node_hi"][at_node])
    return lo, hi


def leaf_count(t, leaf):
    return np.minimum(2, t["n"] - 2 * leaf)


def sah_cost(t):
    c = t["child"]
    lo, hi = child_boxes(t)
    root = max(float(half_area64(t["node_lo"][0], t["node_hi"][0])), 1e-30)
    cost = COST_TRAVERSE * half_area64(t["node_lo"], t["node_hi"]) / root
    for s in range(2):
        leaf = c[:, s] < 0
        cnt = leaf_count(t, np.where(leaf, ~c[:, s], 0))
        cost = cost + np.where(leaf, COST_INTERSECT * cnt * half_area64(lo[:, s], hi[:, s]) / root, 0.0)
    return float(cost.sum())


def _tree(n, order, leaf_lo, leaf_hi, h, rounds, fell_back):
    child, node_lo, node_hi, root_depth = h
    t = {"n": n, "order": order, "leaf_lo": leaf_lo, "leaf_hi": leaf_hi, "child": child, "node_lo": node_lo, "node_hi": node_hi,
         "max_depth": root_depth + 1, "rounds": rounds, "fell_back": fell_back}
    t["cost"] = sah_cost(t)
    return t


def lbvh_tree(lo, hi):
    """Builder 1's tree of the build primitives (lo, hi) [n, 3] float32."""
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    order, leaf_lo, leaf_hi, leaf_keys = sorted_leaves(lo, hi)
    return _tree(len(lo), order, leaf_lo, leaf_hi, lbvh_hierarchy(leaf_lo, leaf_hi, leaf_keys), 0, 0)


def ploc_tree(lo, hi):
    """Builder 2's tree: dict(n, order [n] (the sorted primitives), leaf_lo / leaf_hi [L, 3], child [L-1, 2] (>= 0 node,
    < 0 ~leaf), node_lo / node_hi [L-1, 3] (each node's own box), max_depth, rounds, fell_back, cost (float64))."""
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    order, leaf_lo, leaf_hi, leaf_keys = sorted_leaves(lo, hi)
    h = ploc_hierarchy(leaf_lo, leaf_hi)
    if h is None:
        return _tree(len(lo), order, leaf_lo, leaf_hi, lbvh_hierarchy(leaf_lo, leaf_hi, leaf_keys), MAX_ROUNDS, 1)
    return _tree(len(lo), order, leaf_lo, leaf_hi, h[:4], h[4], 0)


def node_pairs(t):
    """The tree as the L - 1 node pairs the kernels read, [L-1, 16] uint32 (include/p3d_hip.h: p3d_debug_lbvh_build)."""
    c = t["child"]
    lo, hi = child_boxes(t)
    out = np.zeros((len(c), 16), np.uint32)
    f = out.view(F32)
    f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12] = lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]
    leaf = np.where(c < 0, ~c, 0)
    codes = np.where(c < 0, ~(((2 * leaf) << 3) | (leaf_count(t, leaf) - 1)), c)
    out[:, 12:14] = codes.astype(np.int32).view(np.uint32)
    return out
