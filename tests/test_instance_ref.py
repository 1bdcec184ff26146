"""The mesh-instance checker (tests/instance_ref.py) against baked geometry, on the CPU: an instance
of a mesh under T must agree with Mesh.transformed(T) intersected by the oracle as a plain mesh, up
to the rounding of the two routes (transforming the ray against transforming the vertices)."""
import numpy as np
import pytest

import instance_ref as ir
from rrte_amd import Camera, LoweredScene, MeshInstance, Transform, abi, scenes
from rrte_amd.mesh import icosphere, torus

N = 4000
CASES = {
    # name: (mesh, transform, compare normals)
    "icosphere2-rotated-nonuniform": (lambda: icosphere((0.2, 0.1, -0.3), 1.0, 2),
                                      Transform((1.5, 2.0, -1.0), scenes.Q_X45_Y45, (1.7, 0.6, 1.1)), False),
    "torus16x8-rotated-nonuniform": (lambda: torus((0.0, 0.0, 0.0), 1.0, 0.3, 16, 8),
                                     Transform((-2.0, 1.0, 0.5), scenes.Q_X45_Y45, (1.7, 0.6, 1.1)), False),
    "icosphere1-uniform-quarter": (lambda: icosphere((0.0, 1.0, 0.0), 1.0, 1),
                                   Transform((0.5, 0.25, 2.0), scenes.Q_Y45, (0.25, 0.25, 0.25)), True),
}


def rays_into(box_lo, box_hi, seed):
    """N rays from a shell around the box, aimed at points inside it."""
    rng = np.random.default_rng(seed)
    c, half = 0.5 * (box_lo + box_hi), 0.5 * (box_hi - box_lo)
    tg = rng.uniform(box_lo, box_hi, (N, 3))
    u = rng.normal(size=(N, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c + u * (3.0 * np.linalg.norm(half) + 1.0)
    return o.astype(np.float32), (tg - o).astype(np.float32)


@pytest.mark.parametrize("name", list(CASES))
def test_instance_matches_baked_mesh(name):
    """Measured here (4000 rays per case; rays hitting both ways, hit/miss disagreements, max relative
    t difference, max point difference, max normal difference):
      icosphere2-rotated-nonuniform  2636  0  1.85e-6  1.17e-5  (0.036, not asserted)
      torus16x8-rotated-nonuniform   1602  0  4.93e-6  2.68e-5  (2: a grazing hit facing the other way, not asserted)
      icosphere1-uniform-quarter     2969  0  1.75e-6  3.04e-6  1.41e-5
    Under non-uniform scale the interpolated normals legitimately differ (transform-then-interpolate is
    not interpolate-then-transform), so normals are compared for rotation + uniform scale only."""
    make, tr, with_normals = CASES[name]
    mesh = make()
    baked = mesh.transformed(tr)
    o, d = rays_into(baked.positions.min(0).astype(np.float64), baked.positions.max(0).astype(np.float64), 7)
    rays = ir.q.rays_of(o, d)
    inst = LoweredScene([MeshInstance(mesh, tr)], [], Camera())
    flat = LoweredScene([baked], [], Camera())
    got = ir.closest(inst, rays)
    want = ir.closest(flat, rays)
    gh, wh = got["prim"] >= 0, want["prim"] >= 0
    both = gh & wh
    disagree = int((gh != wh).sum())
    rel_t = np.abs(got["t"][both].astype(np.float64) - want["t"][both]) / want["t"][both]
    dp = np.abs(got["point"][both].astype(np.float64) - want["point"][both]).max()
    dn = np.abs(got["normal"][both].astype(np.float64) - want["normal"][both]).max()
    print(f"{name}: hits {int(both.sum())} disagree {disagree} t_rel {rel_t.max():.3g} point {dp:.3g} normal {dn:.3g}")
    assert both.sum() > N // 10
    assert disagree <= 4
    assert rel_t.max() <= 1e-5
    assert dp <= 1e-4
    if with_normals:
        assert dn <= 1e-4


def test_pre_normalised_round_trip():
    rng = np.random.default_rng(3)
    d = ir.normalize_rows(rng.normal(size=(500, 3)).astype(np.float32))
    back = ir.normalize_rows(ir.pre_normalised(d))
    assert np.array_equal(back.view(np.uint32), d.view(np.uint32))


def test_identity_instance_is_the_mesh_up_to_the_ray_transform():
    """An identity transform leaves t_min, t_max and the hit where kind 8 has them (len rounds to 1 or an
    ulp beside it, so t may move by an ulp): the same prims hit, the same triangles."""
    mesh = icosphere((0.0, 1.0, 0.0), 1.0, 1)
    o, d = rays_into(mesh.positions.min(0).astype(np.float64), mesh.positions.max(0).astype(np.float64), 11)
    rays = ir.q.rays_of(o[:200], d[:200])
    a = ir.closest(LoweredScene([MeshInstance(mesh)], [], Camera()), rays)
    b = ir.closest(LoweredScene([mesh], [], Camera()), rays)
    assert np.array_equal(a["prim"], b["prim"]) and (a["prim"] >= 0).sum() > 5
    hit = a["prim"] >= 0
    assert np.array_equal(a["tri"][hit], b["tri"][hit])
    assert np.allclose(a["t"][hit], b["t"][hit], rtol=1e-6, atol=0)
    assert a["prim"].dtype == abi.RAY_HIT_DTYPE["prim"]
