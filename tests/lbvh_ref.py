"""Checker for the device-side BVH build (include/rrte_hip_build.h) -- TEST ONLY, CPU only.

An independent restatement, in numpy float32 and Python integers, of the build's steps 1-5: Morton
cells and codes of the triangles' box centres, the stable sort, 4-triangle leaves and their keys, the
binary radix tree over the leaf keys, and the depths.  The tree is found TOP-DOWN here (split a span
of sorted keys at its highest differing bit) where the library searches bottom-up per record; the
record numbering is the same by definition: a span's left child is record `split`, its right child
record `split + 1`, the root record 0.
"""
import numpy as np

F = np.float32
LEAF_BIT = 0x80000000
NO_PARENT = 0xFFFFFFFF
LEAF_MAX = 4
MAX_RECORDS = 31  # records on a root-to-leaf path the traversal stack takes


# ------------------------------------------------------------------------------- 1. keys
def centres(pos, tris):
    """Box centres 0.5f * (lo + hi) of (n, 3) index triples over (V, 3) float32 positions."""
    p = np.asarray(pos, F)[np.asarray(tris, np.int64)]  # (n, 3 vertices, 3 axes)
    lo, hi = p.min(axis=1), p.max(axis=1)
    return (F(0.5) * (lo + hi).astype(F)).astype(F)


def cells(c, lo, hi):
    """Cells 0..1023 of centres c (n, 3) in the centroid box [lo, hi] (each (3,)), f32 op by op."""
    c, lo, hi = np.asarray(c, F).reshape(-1, 3), np.asarray(lo, F), np.asarray(hi, F)
    q = np.zeros(c.shape, np.int64)
    for a in range(3):
        ext = F(hi[a] - lo[a])
        if not ext > 0:
            continue
        f = ((((c[:, a] - lo[a]).astype(F)) / ext).astype(F) * F(1024.0)).astype(F)
        q[:, a] = np.clip(np.trunc(f.astype(np.float64)), 0, 1023).astype(np.int64)
    return q


def morton(q):
    """30-bit codes of (n, 3) cells: bit 3 i + 2 is bit i of x, 3 i + 1 of y, 3 i of z."""
    out = []
    for x, y, z in np.asarray(q, np.int64).reshape(-1, 3):
        m = 0
        for i in range(10):
            m |= ((int(x) >> i) & 1) << (3 * i + 2) | ((int(y) >> i) & 1) << (3 * i + 1) | ((int(z) >> i) & 1) << (3 * i)
        out.append(m)
    return out


def codes_of(pos, tris):
    """Morton code of every triangle of one range."""
    if len(tris) == 0:
        return []
    c = centres(pos, tris)
    return morton(cells(c, c.min(axis=0), c.max(axis=0)))


# ------------------------------------------------------------------------ 2-3. sort, leaves
def slot_order(codes):
    """Original indices in slot order: by (code, original index)."""
    return sorted(range(len(codes)), key=lambda k: (codes[k], k))


def leaf_keys(sorted_codes):
    """Key of leaf j: (code of its first slot << 32) | j."""
    return [(sorted_codes[LEAF_MAX * j] << 32) | j for j in range((len(sorted_codes) + LEAF_MAX - 1) // LEAF_MAX)]


# ------------------------------------------------------------------------ 4-5. hierarchy, depth
def tree(keys):
    """The radix tree over ascending unique 64-bit keys.  Children are named locally: a leaf j as
    -(j + 1), a record by its index.  Returns a dict of lists over the L - 1 records (child [2], axis,
    parent code or -1, depth, span) and over the leaves (leaf_parent code or -1), and `depth`: the most
    records on a root-to-leaf path."""
    n = len(keys)
    assert all(keys[i] < keys[i + 1] for i in range(n - 1))
    recs = max(n - 1, 0)
    out = {"child": [None] * recs, "axis": [0] * recs, "parent": [-1] * recs, "depth": [0] * recs,
           "span": [None] * recs, "leaf_parent": [-1] * n, "depth_max": 0}
    if n < 2:
        return out
    todo = [(0, 0, n - 1, -1, 0)]
    while todo:
        rec, first, last, parent, depth = todo.pop()
        assert out["span"][rec] is None
        x = keys[first] ^ keys[last]
        bit = x.bit_length() - 1  # the highest bit in which the span's keys differ
        split = first + sum(1 for k in keys[first:last + 1] if not (k >> bit) & 1) - 1
        assert first <= split < last
        out["span"][rec], out["parent"][rec], out["depth"][rec] = (first, last), parent, depth
        out["axis"][rec] = 0 if bit < 32 else 2 - (bit - 32) % 3
        kids = []
        for side, (a, b, idx) in enumerate(((first, split, split), (split + 1, last, split + 1))):
            if a == b:
                kids.append(-(a + 1))
                out["leaf_parent"][a] = rec * 2 + side
            else:
                kids.append(idx)
                todo.append((idx, a, b, rec * 2 + side, depth + 1))
        out["child"][rec] = kids
    out["depth_max"] = max(out["depth"]) + 1
    return out


def check_tree(keys, t):
    """Structural invariants: L - 1 records, every leaf and record reached exactly once from record 0,
    children cover contiguous leaf ranges in order."""
    n = len(keys)
    assert len(t["child"]) == max(n - 1, 0)
    if n < 2:
        return
    seen_rec, seen_leaf = set(), set()

    def cover(node):
        if node < 0:
            j = -node - 1
            assert j not in seen_leaf
            seen_leaf.add(j)
            return j, j
        assert node not in seen_rec
        seen_rec.add(node)
        (a0, b0), (a1, b1) = cover(t["child"][node][0]), cover(t["child"][node][1])
        assert b0 + 1 == a1
        return a0, b1

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * n + 100))
    try:
        assert cover(0) == (0, n - 1)
    finally:
        sys.setrecursionlimit(old)
    assert seen_rec == set(range(n - 1)) and seen_leaf == set(range(n))


# ------------------------------------------------------------------------------ whole scenes
def build_range(pos, tris, slot_base=0, rec_base=0):
    """One range: slot order, the global links / axes / parent codes of its records, its root link and depth."""
    n = len(tris)
    codes = codes_of(pos, tris)
    order = slot_order(codes)
    keys = leaf_keys([codes[k] for k in order])
    t = tree(keys)

    def link(child):
        if child < 0:
            j = -child - 1
            return LEAF_BIT | ((min(LEAF_MAX, n - LEAF_MAX * j) - 1) << 24) | (slot_base + LEAF_MAX * j)
        return rec_base + child

    links = np.array([[link(c) for c in kids] for kids in t["child"]], np.uint32).reshape(-1, 2)
    root = LEAF_BIT if n == 0 else (link(-1) if len(keys) == 1 else rec_base)
    return {"order": np.array(order, np.uint32), "links": links, "axis": np.array(t["axis"], np.uint32), "root": root,
            "depth": t["depth_max"], "codes": codes, "keys": keys, "tree": t}


def scene_ranges(scene):
    """(first, count) of the distinct ranges of a LoweredScene in order of first appearance."""
    seen, out = set(), []
    for i in range(scene.ir.num_prims):
        p = scene.prims[i]
        key = (p.sdf_first, p.sdf_count)
        if p.kind in (8, 9) and key not in seen:
            seen.add(key)
            out.append(key)
    return out


def build_scene(scene):
    """What a device build of `scene` must hold: per-slot original indices, (records, 2) links, axes,
    the depth (most records on a path over all ranges) and the per-range results."""
    idx = np.ctypeslib.as_array(scene.ir.mesh_indices, shape=(scene.ir.num_mesh_indices,)).reshape(-1, 3)
    pos = np.asarray(scene._mesh_vtx, F)[:, :3]
    slots, links, axis, parts, slot_base, rec_base = [], [], [], [], 0, 0
    for first, count in scene_ranges(scene):
        r = build_range(pos, idx[first:first + count], slot_base, rec_base)
        parts.append(r)
        slots.append(r["order"])
        links.append(r["links"])
        axis.append(r["axis"])
        slot_base += count
        rec_base += len(r["links"])
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape, np.uint32)  # noqa: E731
    return {"slots": cat(slots, (0,)), "links": cat(links, (0, 2)), "axis": cat(axis, (0,)),
            "depth": max([r["depth"] for r in parts], default=0), "ranges": parts}
