"""numpy statement of the PLOC builder (option "gpu_builder" = 1; csrc/bvh_ploc.hip): every rule that fixes its bytes, written
independently of the kernels.  The initial cluster order is the LBVH's Morton order, which the callers take from the oracle's
build_mode=1 records (OracleScene(..., build_mode=1).tris()["gid"]).

  clusters   one per triangle, in that order; box = the triangle's vertex box (selects a < b ? a : b), or the point (0, 0, 0)
             where one of its nine coordinates is not finite
  distance   d(i, j) = half area of union(box_i, box_j) in float32: (dx*dy + dy*dz) + dz*dx, no fused multiply-add
  neighbour  NN(i) = argmin of d over j in [i-16, i+16] \\ {i}, candidates in ascending j, the first one kept on ties
  merge      NN(i) = j, NN(j) = i, i < j: new node at position i (left = i, right = j); j dropped; order kept; new nodes of an
             iteration numbered by position
  leaves     a node of <= 4 triangles is a leaf unless kTravCost*A + C(l) + C(r) < count*A; C = count*A for a leaf
  layout     binary nodes in DFS pre-order (root 0, left first), leaves = contiguous leaf-ordered ranges, ref ~((first << 3) | count)
  depth      a kept node at depth 6 whose subtree is taller than 26 becomes a balanced tree over its leaf-ordered triangles
             (left = ceil(count / 2), leaves of <= 4), so every leaf sits at depth <= 32
  small      n <= 4: one leaf of all triangles beside an empty leaf, both with the root box
"""
import numpy as np

F32 = np.float32
RADIUS = 16
LEAF_MAX = 4
MAX_DEPTH = 32
RULE_DEPTH = 6
TRAV_COST = F32(1.0)


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def half_area(box):
    """box (..., 6) = min xyz, max xyz"""
    d = (box[..., 3:] - box[..., :3]).astype(F32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return ((dx * dy + dy * dz) + dz * dx).astype(F32)


def union(a, b):
    return np.concatenate([_min(a[..., :3], b[..., :3]), _max(a[..., 3:], b[..., 3:])], axis=-1).astype(F32)


def tri_boxes(meshes):
    """(n, 6) float32 per gid: min / max of the three vertices as triBoxKernel takes them; all zero for a triangle with a NaN or
    an inf among its nine coordinates"""
    out = []
    for m in meshes:
        t = np.asarray(m["triangles"], dtype=np.int64).reshape(-1, 3)
        if not len(t):
            continue
        v = np.asarray(m["vertices"], dtype=F32).reshape(-1, 3)
        A, B, C = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
        b = np.concatenate([_min(_min(A, B), C), _max(_max(A, B), C)], axis=1)
        b[~np.isfinite(v[t]).all(axis=(1, 2))] = 0  # an inert triangle (crt_hip.h) is the point (0, 0, 0) to every builder
        out.append(b)
    return np.concatenate(out).astype(F32) if out else np.zeros((0, 6), F32)


def nearest_neighbours(cb):
    """NN of every cluster of the current array cb (m, 6)"""
    m = len(cb)
    i = np.arange(m)
    best = np.zeros(m, F32)
    nn = np.full(m, -1, np.int64)
    for off in list(range(-RADIUS, 0)) + list(range(1, RADIUS + 1)):  # ascending j
        j = i + off
        ok = (j >= 0) & (j < m)
        jc = np.clip(j, 0, m - 1)
        d = half_area(union(cb, cb[jc]))
        take = ok & ((nn < 0) | (d < best))
        best = np.where(take, d, best)
        nn = np.where(take, j, nn)
    return nn


def cluster(boxes):
    """the clustering.  boxes (n, 6) in initial order.  Returns the node table (ids < n: the triangles by position) and the
    merges of every iteration as (position i, position j, new id) arrays, for tests of the mutual-NN rule."""
    n = len(boxes)
    tot = 2 * n - 1
    box = np.zeros((tot, 6), F32)
    box[:n] = boxes
    left = np.full(tot, -1, np.int64)
    right = np.full(tot, -1, np.int64)
    count = np.zeros(tot, np.int64)
    count[:n] = 1
    cost = np.zeros(tot, F32)
    cost[:n] = half_area(boxes)
    size = np.zeros(tot, np.int64)
    height = np.zeros(tot, np.int64)
    leaf = np.zeros(tot, bool)
    leaf[:n] = True
    ids = np.arange(n)
    cb = boxes.copy()
    nxt = n
    history = []
    while len(ids) > 1:
        m = len(ids)
        nn = nearest_neighbours(cb)
        pos = np.arange(m)
        mutual = nn[nn] == pos
        merge = mutual & (pos < nn)
        keep = ~(mutual & (pos > nn))
        mi = np.nonzero(merge)[0]
        if not len(mi):
            raise RuntimeError("no mutual neighbours")
        mj = nn[mi]
        new = nxt + np.arange(len(mi))
        L, R = ids[mi], ids[mj]
        b = union(cb[mi], cb[mj])
        A = half_area(b)
        cnt = count[L] + count[R]
        inner = ((TRAV_COST * A + cost[L]) + cost[R]).astype(F32)
        as_leaf = (cnt.astype(F32) * A).astype(F32)
        lf = (cnt <= LEAF_MAX) & ~(inner < as_leaf)
        box[new], left[new], right[new], count[new] = b, L, R, cnt
        cost[new] = np.where(lf, as_leaf, inner)
        size[new] = np.where(lf, 0, 1 + size[L] + size[R])
        height[new] = np.where(lf, 0, 1 + np.maximum(height[L], height[R]))
        leaf[new] = lf
        history.append((mi, mj, new))
        nxt += len(mi)
        ids = ids.copy()
        ids[mi] = new
        cb = cb.copy()
        cb[mi] = b
        ids, cb = ids[keep], cb[keep]
    return dict(n=n, box=box, left=left, right=right, count=count, cost=cost, size=size, height=height, leaf=leaf,
                root=nxt - 1, history=history)


def _leafref(first, cnt):
    return ~((first << 3) | cnt)


def _fold(boxes):
    b = boxes[0]
    for k in range(1, len(boxes)):
        b = union(b, boxes[k])
    return b


def build(boxes_by_gid, order, node_dtype):
    """The PLOC tree of the triangles `order` (gids, in the initial order) with boxes boxes_by_gid.  Returns (nodes, gid_order,
    max_depth, table): binary nodes as node_dtype in DFS pre-order, the gids in leaf order, the deepest leaf (root = 0) and the
    clustering (cluster())."""
    order = np.asarray(order, dtype=np.int64)
    boxes_by_gid = np.asarray(boxes_by_gid, dtype=F32)
    n = len(order)
    nodes = []
    if n == 0:
        return np.zeros(0, node_dtype), order, 0, None
    if n <= LEAF_MAX:
        root = _fold(boxes_by_gid[np.arange(n)])  # (folded in gid order, as the builders' host path does)
        rec = (root, root, _leafref(0, n), ~0)
        return _records([rec], node_dtype), order, 1, None
    T = cluster(boxes_by_gid[order])
    box, left, right, count, leaf, height = T["box"], T["left"], T["right"], T["count"], T["leaf"], T["height"]
    tri_order = []  # positions (< n) in leaf order

    def leaves_of(x):
        out, stack = [], [x]
        while stack:
            y = stack.pop()
            if y < n:
                out.append(y)
            else:
                stack.append(right[y])
                stack.append(left[y])
        return out

    def leaf_child(c):
        first = len(tri_order)
        tri_order.extend(leaves_of(c))
        return _leafref(first, int(count[c]))

    def balanced(first, cnt):
        me = len(nodes)
        nodes.append(None)
        half = (cnt + 1) // 2
        parts = []
        for f, c in ((first, half), (first + half, cnt - half)):
            b = _fold(boxes_by_gid[order[tri_order[f:f + c]]])
            parts.append((b, _leafref(f, c) if c <= LEAF_MAX else balanced(f, c)))
        nodes[me] = (parts[0][0], parts[1][0], parts[0][1], parts[1][1])
        return me

    def visit(x, depth):
        if depth == RULE_DEPTH and height[x] > MAX_DEPTH - RULE_DEPTH:
            first = len(tri_order)
            tri_order.extend(leaves_of(x))
            return balanced(first, int(count[x]))
        me = len(nodes)
        nodes.append(None)
        refs = []
        for c in (left[x], right[x]):
            refs.append(leaf_child(c) if (c < n or leaf[c]) else visit(c, depth + 1))
        nodes[me] = (box[left[x]], box[right[x]], refs[0], refs[1])
        return me

    visit(T["root"], 0)
    out = _records(nodes, node_dtype)
    return out, order[np.asarray(tri_order, dtype=np.int64)], max_depth(out), T


def _records(recs, node_dtype):
    out = np.zeros(len(recs), node_dtype)
    for k, (lb, rb, lr, rr) in enumerate(recs):
        for a, ax in enumerate("xyz"):
            out[k]["l%s0" % ax], out[k]["l%s1" % ax] = lb[a], lb[3 + a]
            out[k]["r%s0" % ax], out[k]["r%s1" % ax] = rb[a], rb[3 + a]
        out[k]["left"], out[k]["right"] = lr, rr
    return out


def max_depth(nodes):
    """deepest child reference of the binary tree (root = depth 0): what crt_bvh_info reports as max_depth"""
    if not len(nodes):
        return 0
    deepest, stack = 0, [(0, 0)]
    while stack:
        b, d = stack.pop()
        deepest = max(deepest, d + 1)
        for ch in (int(nodes[b]["left"]), int(nodes[b]["right"])):
            if ch >= 0:
                stack.append((ch, d + 1))
    return deepest


def child_boxes(nodes):
    """(m, 2, 6): the left and right child boxes of every binary node"""
    f = lambda k: nodes[k].astype(F32)  # noqa: E731
    lb = np.stack([f("lx0"), f("ly0"), f("lz0"), f("lx1"), f("ly1"), f("lz1")], 1)
    rb = np.stack([f("rx0"), f("ry0"), f("rz0"), f("rx1"), f("ry1"), f("rz1")], 1)
    return np.stack([lb, rb], 1)


def sah_cost(nodes):
    """SAH cost of a binary tree, relative to its root box: sum of kTravCost * A over inner nodes + count * A over leaves"""
    cb = child_boxes(nodes).astype(np.float64)
    A = lambda b: (lambda d: d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])(b[..., 3:] - b[..., :3])  # noqa: E731
    root = np.concatenate([np.minimum(cb[0, 0, :3], cb[0, 1, :3]), np.maximum(cb[0, 0, 3:], cb[0, 1, 3:])])
    ar = A(root)
    total = ar * float(TRAV_COST)  # the root
    refs = np.stack([nodes["left"], nodes["right"]], 1).astype(np.int64)
    areas = A(cb)
    inner = refs >= 0
    total += float(TRAV_COST) * areas[inner].sum()
    cnt = (~refs[~inner]) & 7
    total += (cnt * areas[~inner]).sum()
    return total / ar if ar > 0 else 0.0
