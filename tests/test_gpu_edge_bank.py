"""The device's ray queries over the edge-case ray bank (tests/edge_bank.py): for every tier and object
group rrte_hip_raycast in its CLOSEST and ANY form against the oracle loop
(query_ref.oracle_closest / oracle_any; instance_ref for mesh instances), through
query_ref.assert_hits_equal -- prim, front face and material equal, t, point and normal bit-identical
or NaN on both sides.  The tiers run in the bank's order: lattice, interval, ties, scales, then the
two degenerate tiers.  tests/test_edge_bank_cpu.py checks the checker on the same cases.

The random-ray tests cap the oracle's non-finite records at 1 %; here they are the point, so each
case asserts the count the CPU test established (edge_bank.NON_FINITE) instead."""
import ctypes as C

import numpy as np
import pytest

import edge_bank as eb
import query_ref as q
from rrte_amd import Camera, Context, LoweredScene, Raytracer, RaytracerConfig, Sphere, abi

pytestmark = pytest.mark.gpu

IDS = [f"{t}-{g}" for t, g in eb.CASES]


@pytest.fixture(scope="module")
def rt():
    r = Raytracer(device=0)
    yield r
    r.ctx.close()


def _raycast(ctx, sc, rays, any_hit):
    hits = np.zeros(len(rays), dtype=abi.RAY_HIT_DTYPE)
    ctx.check(ctx.lib.rrte_hip_raycast(ctx.h, sc.ref(), rays.ctypes.data_as(C.POINTER(abi.Ray)), len(rays),
                                       abi.QUERY_ANY if any_hit else abi.QUERY_CLOSEST,
                                       hits.ctypes.data_as(C.POINTER(abi.RayHit))))
    return hits


def check(tier, group, got, want, tri):
    try:
        q.assert_hits_equal(got, want, tri=tri)
    except AssertionError as e:
        bad = e.args[0][1] if e.args and isinstance(e.args[0], tuple) else []
        raise AssertionError(f"{e}\nrays: {eb.describe(tier, group, bad)}") from None


@pytest.mark.parametrize("tier,group", eb.CASES, ids=IDS)
def test_queries_match_the_oracle(rt, tier, group):
    _, _, rays, _, sc = eb.case(tier, group)
    wc, wa = eb.want_closest(tier, group), eb.want_any(tier, group)
    hits = int((wc["prim"] >= 0).sum())
    print(f"{tier}/{group}: rays {len(rays)} hits {hits} misses {len(rays) - hits} "
          f"non-finite {int(eb.non_finite(wc).sum())} occluded {int((wa['prim'] >= 0).sum())}")
    assert int(eb.non_finite(wc).sum()) == eb.NON_FINITE[(tier, group)]
    # (instance_ref fills `tri`, the plain oracle loop leaves it 0)
    check(tier, group, _raycast(rt.ctx, sc, rays, False), wc, tri=eb.has_instance(sc))
    check(tier, group, _raycast(rt.ctx, sc, rays, True), wa, tri=True)


def test_the_confirmed_any_hit_divergence(rt):
    """(3e19, 0, 0) -> (1, 0, 0) against the unit sphere, t in [1e-3, inf): the reference reports a hit
    (t = NaN: hb*hb and a*cc both overflow), so RRTE_QUERY_ANY must report the sphere.  The any-hit
    early-out for rays leaving a sphere answered "miss" here before it was bounded by hb < 2^63."""
    objs = [eb.analytic("sphere")]
    rays = q.rays_of(np.array([[3e19, 0, 0], [3e18, 0, 0]], np.float32), np.array([[1, 0, 0], [1, 0, 0]], np.float32))
    sc = LoweredScene(objs, [], Camera())
    wa, wc = q.oracle_any(sc, rays), q.oracle_closest(sc, rays)
    assert list(wa["prim"]) == [0, -1] and np.isnan(wc["t"][0])
    q.assert_hits_equal(_raycast(rt.ctx, sc, rays, True), wa, tri=True)
    q.assert_hits_equal(_raycast(rt.ctx, sc, rays, False), wc)


@pytest.mark.parametrize("how", ["host", "device", "refit"])
def test_duplicated_triangles_the_lowest_index_wins(how):
    """A mesh that lists every triangle twice, its shared edges and vertices hit dead on: the hit is
    the one of the same triangles listed one by one, and `tri` names the lower index of the pair --
    under the HOST and the DEVICE build policy, and after rrte_hip_mesh_refit with unchanged vertices."""
    objs, _, rays, _, sc = eb.case("ties", "dup_mesh")
    want = eb.want_closest("ties", "dup_mesh_triangles")  # prim = the triangle's index
    hit = want["prim"] >= 0
    assert hit.sum() >= 100 and (want["prim"][hit] % 2 == 0).all() and len(set(want["prim"][hit])) == 8
    ctx = Context(0)
    ctx.set_mesh_build(abi.MESH_BUILD_DEVICE if how == "device" else abi.MESH_BUILD_HOST)
    got = _raycast(ctx, sc, rays, False)
    if how == "device":
        assert ctx.build_info().device_builds == 1
    if how == "refit":
        sc = LoweredScene(objs, [], Camera())
        ctx.mesh_refit(sc)
        got = _raycast(ctx, sc, rays, False)
        assert ctx.refit_info().device_refits == 1 and ctx.mesh_info().bvh_builds == 1
    assert np.array_equal(got["prim"] >= 0, hit)
    assert np.array_equal(got["tri"][hit], want["prim"][hit]) and not got["tri"][~hit].any()
    for f in ("t", "point", "normal"):
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)), f
    assert np.array_equal(got["front_face"], want["front_face"])
    ctx.close()


@pytest.mark.parametrize("group", list(eb.REJECTED_OBJECTS))
def test_rejected_objects_return_their_status_and_write_nothing(rt, group):
    _, _, rays, _ = eb.tier_degenerate_objects(group)
    objs = eb.REJECTED_OBJECTS[group]()
    sc = LoweredScene(objs, [], Camera())
    hits = np.zeros(len(rays), dtype=abi.RAY_HIT_DTYPE)
    hits.view(np.uint8)[:] = 0xA5
    for flags in (abi.QUERY_CLOSEST, abi.QUERY_ANY):
        st = rt.ctx.lib.rrte_hip_raycast(rt.ctx.h, sc.ref(), rays.ctypes.data_as(C.POINTER(abi.Ray)), len(rays), flags,
                                         hits.ctypes.data_as(C.POINTER(abi.RayHit)))
        assert st == abi.RRTE_INVALID_ARG
        assert (hits.view(np.uint8) == 0xA5).all()
    # the context still answers
    objs = [Sphere((0, 0, 0), 1.0)]
    got = rt.raycast(objs, [[0, 0, 3]], [[0, 0, -1]])
    assert got["prim"][0] == 0 and got["t"][0] == np.float32(2.0)


def ortho_frame(w=16, h=16):
    """The exact orthographic frame: Camera.new_orthographic(-2, 2, -2, 2) at (0, 0, 8) looking down
    -z (the identity rotation), 16x16 pixels.  Every pixel ray is exactly (0, 0, -1) with its origin
    on the 1/8 lattice, and the unit sphere centred at (0.125, 0.125, 0.125) has exactly tangent ones."""
    cam = Camera.new_orthographic(-2.0, 2.0, -2.0, 2.0, 0.1, 100.0)
    cam.transform.position = (np.float32(0), np.float32(0), np.float32(8))
    cfg = RaytracerConfig(width=w, height=h, samples_per_pixel=1, max_depth=1, jitter="center")
    return cam, cfg


def test_pick_on_the_exact_orthographic_frame():
    w = h = 16
    cam, cfg = ortho_frame(w, h)
    objs = [Sphere((0.125, 0.125, 0.125), 1.0, eb.MAT), eb.analytic("cube", "exact")]
    ys, xs = np.divmod(np.arange(w * h), w)
    sc = LoweredScene(objs, [], cam)
    rays = q.oracle_pick_rays(sc, w, h, xs, ys, cfg.t_min)
    assert (rays["direction"] == np.array([0, 0, -1], np.float32)).all()
    assert (np.modf(rays["origin"] * 8)[0] == 0).all()  # origins on the 1/8 lattice
    want = q.oracle_closest(sc, rays)
    on_sphere = want["prim"] == 0
    # tangent pixel rays: disc == 0, the largest hit t = 8 - 0.125
    assert on_sphere.sum() >= 40 and want["t"][on_sphere].max() == np.float32(7.875)
    oc = rays["origin"] - np.float32(0.125)
    disc = oc[:, 2] * oc[:, 2] - ((oc * oc).sum(1, dtype=np.float32) - np.float32(1))
    assert ((disc == 0) & on_sphere).sum() >= 3  # (the cube hides the fourth)
    rt = Raytracer(cfg, device=0)
    q.assert_hits_equal(rt.pick(objs, cam, xs, ys), want)
    rt.ctx.close()
