"""Checker for the device-side BVH refit (include/rrte_hip_refit.h, rrte_amd/csrc/mesh_refit.hip) --
TEST ONLY, CPU only.

A numpy float32 restatement of what the refit kernels compute from a node array (the 64-byte interior
records rrte_hip_mesh_nodes returns), the slot -> vertex table and the deformed positions: every leaf's
box is the union of its triangles' boxes over their VERTEX POSITIONS, inflated; every interior box is
the exact union of its two children's.  Each min / max is the compare-and-select of the C++ (the first
operand wins a tie, so signed zeros come out the same), each f32 operation is rounded on its own.
"""
import numpy as np

F = np.float32
LEAF_BIT = 0x80000000
INF = F(np.inf)


def grow(lo, hi, plo, phi):
    """Box::grow: lo = p < lo ? p : lo, hi = hi < p ? p : hi (element-wise, any leading shape)."""
    return np.where(plo < lo, plo, lo).astype(F), np.where(hi < phi, phi, hi).astype(F)


def empty_box(shape=()):
    return np.full(shape + (3,), INF, F), np.full(shape + (3,), -INF, F)


def inflate(lo, hi):
    """mesh_box.hpp inflate() on (..., 3) float32 boxes."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    ext = np.zeros(lo.shape[:-1], F)
    mag = np.zeros(lo.shape[:-1], F)
    with np.errstate(all="ignore"):
        for k in range(3):
            e = (hi[..., k] - lo[..., k]).astype(F)
            ext = np.where(ext < e, e, ext).astype(F)
            al, ah = np.abs(lo[..., k]), np.abs(hi[..., k])
            m = np.where(al < ah, ah, al).astype(F)
            mag = np.where(mag < m, m, mag).astype(F)
        d = ((F(1e-2) * ext).astype(F) + (F(1e-5) * mag).astype(F)).astype(F)
        d = (d + F(1e-6)).astype(F)
        out_lo = np.nextafter((lo - d[..., None]).astype(F), -INF).astype(F)
        out_hi = np.nextafter((hi + d[..., None]).astype(F), INF).astype(F)
    return out_lo, out_hi


def leaf_slots(link):
    """(first slot, count) of a leaf link: count - 1 in bits 24-30 (1..128), first slot in bits 0-23."""
    link = int(link)
    assert link & LEAF_BIT
    return link & 0xFFFFFF, ((link >> 24) & 0x7F) + 1


def leaf_box(link, slot_vtx, pos):
    """The un-inflated box of a leaf: per slot the box over v0, v1, v2 in that order, united in slot order."""
    a, n = leaf_slots(link)
    lo, hi = empty_box()
    for k in range(a, a + n):
        tlo, thi = empty_box()
        for j in range(3):
            p = pos[slot_vtx[k, j]]
            tlo, thi = grow(tlo, thi, p, p)
        lo, hi = grow(lo, hi, tlo, thi)
    return lo, hi


def links_of(nodes):
    """(records, 2) uint32 child links of a (records, 4, 4) float32 node array."""
    u = np.ascontiguousarray(nodes, dtype=F).view(np.uint32)
    return u[:, (0, 2), 3]


def roots_of(nodes):
    """The records that are nobody's child: one per range whose root is not a leaf."""
    links = links_of(nodes)
    kids = {int(x) for x in links.reshape(-1) if not int(x) & LEAF_BIT}
    return [r for r in range(len(nodes)) if r not in kids]


def refit(nodes, slot_vtx, pos):
    """The node array after a refit to `pos` ((V, 3) float32): links and the other w words kept."""
    nodes = np.ascontiguousarray(nodes, dtype=F)
    pos = np.asarray(pos, F)
    out = nodes.copy()
    links = links_of(nodes)

    def box(link):
        link = int(link)
        if link & LEAF_BIT:
            return inflate(*leaf_box(link, slot_vtx, pos))
        b0, b1 = box(links[link, 0]), box(links[link, 1])
        out[link, 0, :3], out[link, 1, :3] = b0
        out[link, 2, :3], out[link, 3, :3] = b1
        return grow(b0[0], b0[1], b1[0], b1[1])

    tops = {}
    for r in roots_of(nodes):
        tops[r] = box(r)
    return out, tops


def slot_vertex_table(scene, slots):
    """(slots, 3) vertex indices from Context.mesh_slots() (each slot's triangle index within its range)
    and a LoweredScene: ranges lie in the slot array in order of first appearance in the object list."""
    idx = np.ctypeslib.as_array(scene.ir.mesh_indices, shape=(scene.ir.num_mesh_indices,)).reshape(-1, 3)
    seen, base, out = set(), 0, np.zeros((len(slots), 3), np.uint32)
    for i in range(scene.ir.num_prims):
        p = scene.prims[i]
        key = (p.sdf_first, p.sdf_count)
        if p.kind not in (8, 9) or key in seen:
            continue
        seen.add(key)
        out[base:base + p.sdf_count] = idx[p.sdf_first + np.asarray(slots[base:base + p.sdf_count], np.int64)]
        base += p.sdf_count
    assert base == len(slots)
    return out


def synthetic_tree():
    """A 3-level tree over 7 triangles / 21 vertices: record 0 = (record 1, record 2), record 1 =
    (leaf of 2 slots, leaf of 1), record 2 = (leaf of 3 slots -- count field 2 --, leaf of 1).
    Returns (nodes with stale boxes, slot_vtx)."""
    nodes = np.zeros((3, 4, 4), F)
    u = nodes.view(np.uint32)

    def leaf(first, n):
        return LEAF_BIT | ((n - 1) << 24) | first
    u[0, 0, 3], u[0, 2, 3] = 1, 2
    u[1, 0, 3], u[1, 2, 3] = leaf(0, 2), leaf(2, 1)
    u[2, 0, 3], u[2, 2, 3] = leaf(3, 3), leaf(6, 1)
    u[:, 1, 3] = (0, 2, 1)  # split axes: w words a refit keeps
    nodes[:, :, :3] = F(123.0)  # stale boxes
    slot_vtx = np.arange(21, dtype=np.uint32).reshape(7, 3)[::-1].copy()
    return nodes, slot_vtx
