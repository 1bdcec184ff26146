"""Deforming meshes without a GPU: Mesh.set_vertices, and the refit checker tests/refit_ref.py on
its own -- inflate() is monotone (the containment argument of DESIGN.md §17 rests on it), and on a
synthetic 3-level tree with a 3-triangle leaf every parent box contains its children's and every leaf
box its vertices."""
import numpy as np
import pytest

import refit_ref as rr
from rrte_amd import LoweredScene, Camera
from rrte_amd.mesh import Mesh, face_normals, heightfield, icosphere, normalize_rows

F = np.float32


# ------------------------------------------------------------------------------ Mesh.set_vertices
def _quad():
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]], F)
    return Mesh(pos, np.array([[0, 2, 1], [0, 3, 2]], np.uint32))


def test_set_vertices_refuses_other_shapes_and_dtypes():
    m = _quad()
    before = m.positions.copy()
    for bad in (np.zeros((3, 3), F), np.zeros((5, 3), F), np.zeros((4, 2), F), np.zeros(12, F), np.zeros((4, 3, 1), F)):
        with pytest.raises(ValueError):
            m.set_vertices(bad)
    with pytest.raises(ValueError):
        m.set_vertices(np.zeros((4, 3), F), normals=np.zeros((3, 3), F))
    with pytest.raises(ValueError):
        m.set_vertices(np.array([["a"] * 3] * 4))
    with pytest.raises(ValueError):
        m.set_vertices(np.zeros((4, 3), F), normals=np.zeros((4, 3), bool))
    with pytest.raises(ValueError):
        m.set_vertices(np.zeros((4, 3), complex))
    assert np.array_equal(m.positions, before)  # a refused call changes nothing


def test_set_vertices_converts_copies_and_recomputes_normals():
    m = _quad()
    assert np.array_equal(m.normals, np.tile(np.array([0, 1, 0], F), (4, 1)))
    new = np.array([[0, 0, 0], [1, 1, 0], [1, 1, 1], [0, 0, 1]], np.float64)  # tilted 45 degrees about z
    m.set_vertices(new)
    assert m.positions.dtype == F and m.positions.flags.c_contiguous and m.positions.shape == (4, 3)
    new[0, 0] = 99.0
    assert m.positions[0, 0] == 0.0
    # the constructor's rule: area-weighted face normals accumulated per vertex, then normalised
    want = Mesh(m.positions, m.indices).normals
    assert np.array_equal(m.normals.view(np.uint32), want.view(np.uint32))
    s = F(1.0) / np.sqrt(F(2.0))
    assert np.allclose(m.normals, np.tile(np.array([-s, s, 0], F), (4, 1)), atol=1e-6)
    fn = face_normals(m.positions, m.indices)
    assert np.allclose(fn, m.normals[:2], atol=1e-6)
    # given normals are normalised as the constructor normalises them
    given = np.tile(np.array([0.0, 3.0, 4.0]), (4, 1))
    m.set_vertices(m.positions, normals=given)
    assert np.array_equal(m.normals.view(np.uint32), normalize_rows(given.astype(F)).view(np.uint32))
    assert m.indices.shape == (2, 3)


def test_a_deformed_mesh_lowers_with_the_same_topology():
    ball = icosphere((0.0, 1.0, 0.0), 1.0, 1)
    a = LoweredScene([ball], [], Camera())
    ia = np.ctypeslib.as_array(a.ir.mesh_indices, shape=(a.ir.num_mesh_indices,)).copy()
    ball.set_vertices(ball.positions * F(1.5) + F(2.0))
    b = LoweredScene([ball], [], Camera())
    ib = np.ctypeslib.as_array(b.ir.mesh_indices, shape=(b.ir.num_mesh_indices,))
    assert np.array_equal(ia, ib) and a.ir.num_mesh_vertices == b.ir.num_mesh_vertices
    assert a.ir.mesh_version != b.ir.mesh_version
    vb = np.ctypeslib.as_array(C_float_ptr(b), shape=(b.ir.num_mesh_vertices, 6))
    assert np.array_equal(vb[:, :3], ball.positions) and np.array_equal(vb[:, 3:], ball.normals)


def C_float_ptr(sc):
    import ctypes as C
    return C.cast(sc.ir.mesh_vertices, C.POINTER(C.c_float))


# -------------------------------------------------------------------------------------- inflate
def test_inflate_matches_a_scalar_restatement_and_signed_zeros_survive():
    lo, hi = np.array([-0.0, 1.0, -3.0], F), np.array([0.0, 1.0, 5.0], F)
    ilo, ihi = rr.inflate(lo, hi)
    d = F(F(F(1e-2) * F(8.0)) + F(F(1e-5) * F(5.0))) + F(1e-6)
    assert d.dtype == F
    for k in range(3):
        assert ilo[k] == np.nextafter(F(lo[k] - d), F(-np.inf)) and ihi[k] == np.nextafter(F(hi[k] + d), F(np.inf))
    assert (ilo < lo).all() and (ihi > hi).all()
    # a degenerate box at the origin still grows: the absolute term and the outward ulp
    zlo, zhi = rr.inflate(np.zeros(3, F), np.zeros(3, F))
    assert (zlo < 0).all() and (zhi > 0).all()
    # compare-and-select keeps the first operand on a tie: -0 then +0 stays -0, and the other way round
    a, _ = rr.grow(np.array([-0.0] * 3, F), np.array([-0.0] * 3, F), np.array([0.0] * 3, F), np.array([0.0] * 3, F))
    b, _ = rr.grow(np.array([0.0] * 3, F), np.array([0.0] * 3, F), np.array([-0.0] * 3, F), np.array([-0.0] * 3, F))
    assert np.signbit(a).all() and not np.signbit(b).any()


def test_inflate_is_monotone_on_random_boxes():
    rng = np.random.default_rng(20261019)
    n = 20000
    scale = (10.0 ** rng.uniform(-6, 6, (n, 1))).astype(F)
    c = (rng.uniform(-1, 1, (n, 3)) * scale).astype(F)
    half = (rng.uniform(0, 1, (n, 3)) * scale * 10.0 ** rng.uniform(-4, 0, (n, 1))).astype(F)
    wlo, whi = (c - half).astype(F), (c + half).astype(F)
    # a part: any box inside the whole, degenerate ones and ones touching the whole's faces included
    u, v = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3))
    u[: n // 8], v[: n // 8] = 0.0, 1.0
    v[n // 8: n // 4] = u[n // 8: n // 4]
    t0, t1 = np.minimum(u, v), np.maximum(u, v)
    plo = np.clip((wlo + (whi - wlo) * t0).astype(F), wlo, whi)
    phi = np.clip((wlo + (whi - wlo) * t1).astype(F), plo, whi)
    assert (plo >= wlo).all() and (phi <= whi).all() and (plo <= phi).all()
    iwlo, iwhi = rr.inflate(wlo, whi)
    iplo, iphi = rr.inflate(plo, phi)
    assert (iwlo <= iplo).all() and (iwhi >= iphi).all()
    assert (iwlo < wlo).all() and (iwhi > whi).all()


# ------------------------------------------------------------------------------- synthetic tree
def test_refit_of_a_synthetic_tree_is_conservative_and_keeps_the_links():
    nodes, slot_vtx = rr.synthetic_tree()
    rng = np.random.default_rng(7)
    pos = (rng.uniform(-3, 3, (21, 3)) + np.array([40.0, -7.0, 0.0])).astype(F)
    pos[5, 1] = F(-0.0)
    out, tops = rr.refit(nodes, slot_vtx, pos)
    assert np.array_equal(out.view(np.uint32)[:, :, 3], nodes.view(np.uint32)[:, :, 3])  # links, axes
    assert rr.roots_of(nodes) == [0] and list(tops) == [0]
    assert not (out[:, :, :3] == F(123.0)).any()  # every stale box was overwritten
    links = rr.links_of(nodes)
    assert rr.leaf_slots(links[2, 0]) == (3, 3)  # the count field above 1

    def contains(lo, hi, plo, phi):
        return (lo <= plo).all() and (hi >= phi).all()
    n_leaves = 0
    for r in range(3):
        for side in range(2):
            lo, hi = out[r, 2 * side, :3], out[r, 2 * side + 1, :3]
            link = int(links[r, side])
            if link & rr.LEAF_BIT:
                a, n = rr.leaf_slots(link)
                n_leaves += 1
                p = pos[slot_vtx[a:a + n].reshape(-1)]
                assert (lo < p.min(0)).all() and (hi > p.max(0)).all()
                ulo, uhi = rr.leaf_box(link, slot_vtx, pos)
                assert np.array_equal(ulo, p.min(0)) and np.array_equal(uhi, p.max(0))
            else:
                for s2 in range(2):  # the slot of `link` in r holds exactly the union of link's two children
                    assert contains(lo, hi, out[link, 2 * s2, :3], out[link, 2 * s2 + 1, :3])
                assert np.array_equal(lo, np.minimum(out[link, 0, :3], out[link, 2, :3]))
                assert np.array_equal(hi, np.maximum(out[link, 1, :3], out[link, 3, :3]))
    assert n_leaves == 4
    # the root's union contains every vertex; the host's culling box (inflate of the box over all
    # vertices) contains the root's union
    tlo, thi = tops[0]
    assert (tlo < pos.min(0)).all() and (thi > pos.max(0)).all()
    hlo, hhi = rr.inflate(pos.min(0), pos.max(0))
    assert contains(hlo, hhi, tlo, thi)


def test_refit_of_unchanged_vertices_is_idempotent():
    nodes, slot_vtx = rr.synthetic_tree()
    pos = np.linspace(-2, 2, 63, dtype=F).reshape(21, 3)
    once, _ = rr.refit(nodes, slot_vtx, pos)
    twice, _ = rr.refit(once, slot_vtx, pos)
    assert np.array_equal(once.view(np.uint32), twice.view(np.uint32))


def test_slot_vertex_table_follows_the_ranges():
    a = icosphere((0.0, 1.0, 0.0), 1.0, 0)
    b = heightfield((0.0, 0.0, 0.0), 1.0, 3, lambda x, z: 0.0 * x)
    sc = LoweredScene([a, b, a], [], Camera())
    slots = np.concatenate([np.arange(20)[::-1], np.arange(8)]).astype(np.uint32)
    tab = rr.slot_vertex_table(sc, slots)
    assert tab.shape == (28, 3)
    assert np.array_equal(tab[:20], a.indices[::-1])
    assert np.array_equal(tab[20:], b.indices + len(a.positions))
