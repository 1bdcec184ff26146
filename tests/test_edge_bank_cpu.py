"""The checker first: on every case of the edge-case ray bank (tests/edge_bank.py) the C oracle's loop
(query_ref.oracle_closest) and the numpy restatement (numpy_ref.intersect / sdf_march /
sdf_attributes, written from the reference's source, not from the oracle) must agree bit for bit on
hit/miss, t, point, normal and front face -- a NaN on both sides counting as equal.  Where the two
disagreed neither would be the authority.  Meshes, which numpy_ref does not restate, compare the
oracle's linear scan with the same triangles listed one by one; a mesh instance's checker
(instance_ref) is itself built from the two and is only counted here.

The bank must not pass vacuously: the counts asserted at the end come from the oracle's answers
alone and are printed.  CPU only."""
import functools

import numpy as np
import pytest

import edge_bank as eb
import numpy_ref as nr
import query_ref as q
from rrte_amd import Camera, LoweredScene, abi

F = np.float32
IDS = [f"{t}-{g}" for t, g in eb.CASES]


def numpy_closest(sc, rays):
    """query_ref.oracle_closest's loop over numpy_ref.intersect: Ray::new's normalisation, list order,
    strict '<', an SDF object marched up to min(t_max, best t) once a hit exists."""
    n = len(rays)
    with np.errstate(all="ignore"):
        d = q._ray_new_direction(rays["direction"])
    o = [np.ascontiguousarray(rays["origin"][:, k]) for k in range(3)]
    dd = [np.ascontiguousarray(d[:, k]) for k in range(3)]
    nodes = [sc.nodes[i] for i in range(sc.ir.num_sdf_nodes)]
    out = np.zeros(n, dtype=abi.RAY_HIT_DTYPE)
    out[:] = q.miss_record()
    found = np.zeros(n, bool)
    best_t = np.full(n, np.inf, F)
    for i in range(sc.ir.num_prims):
        pr = sc.prims[i]
        tmax = rays["t_max"].astype(F)
        with np.errstate(invalid="ignore"):
            if pr.kind == abi.PRIM_SDF:
                tmax = np.where(found, np.where(tmax < best_t, tmax, best_t), tmax).astype(F)
            h = nr.intersect(pr, o, dd, rays["t_min"].astype(F), tmax, nodes)
            better = h.ok & (~found | (h.t < best_t))
        out["t"][better], out["prim"][better], out["material"][better] = h.t[better], i, pr.material
        out["point"][better] = np.stack(h.p, 1)[better]
        out["normal"][better] = np.stack(h.n, 1)[better]
        out["front_face"][better] = h.front[better]
        best_t = np.where(better, h.t, best_t)
        found |= better
    return out


def triangles_closest(tier, group):
    """The case's meshes listed triangle by triangle, through the oracle loop; also each record's
    object index mapped back to (mesh object, triangle)."""
    objs, lights, rays, _, _ = eb.case(tier, group)
    flat, owner = [], []
    for k, o in enumerate(objs):
        tris = o.triangles() if hasattr(o, "triangles") else [o]
        flat += tris
        owner += [k] * len(tris)
    w = q.oracle_closest(LoweredScene(flat, lights, Camera()), rays)
    return w, np.array(owner)


def has_mesh(sc):
    return any(sc.prims[i].kind == abi.PRIM_MESH for i in range(sc.ir.num_prims))


@pytest.mark.parametrize("tier,group", eb.CASES, ids=IDS)
def test_oracle_and_numpy_agree(tier, group):
    _, _, rays, labels, sc = eb.case(tier, group)
    want = eb.want_closest(tier, group)
    hits = int((want["prim"] >= 0).sum())
    print(f"{tier}/{group}: rays {len(rays)} hits {hits} misses {len(rays) - hits} "
          f"non-finite {int(eb.non_finite(want).sum())}")
    assert len(labels) == len(rays) > 0
    assert int(eb.non_finite(want).sum()) == eb.NON_FINITE[(tier, group)]
    if eb.has_instance(sc):
        return
    try:
        if has_mesh(sc):
            other, owner = triangles_closest(tier, group)
            other = other.copy()
            hit = other["prim"] >= 0
            other["prim"][hit] = owner[other["prim"][hit]]
        else:
            other = numpy_closest(sc, rays)
        q.assert_hits_equal(other, want)
    except AssertionError as e:
        bad = e.args[0][1] if e.args and isinstance(e.args[0], tuple) else []
        raise AssertionError(f"{e}\nrays: {eb.describe(tier, group, bad)}") from None


def test_any_is_closest_has_a_hit_without_sdf():
    """The checker itself: without SDF objects (whose interval shrinks once a hit exists) a ray is
    occluded exactly where it has a closest hit, and ANY names the lowest index that hits."""
    for tier, group in [("lattice", "cube/exact"), ("ties", "plane_cube"), ("ties", "dup_mesh"),
                        ("scales", "far/sphere"), ("degenerate_rays", "triangle"), ("interval", "capsule")]:
        wc, wa = eb.want_closest(tier, group), eb.want_any(tier, group)
        assert np.array_equal(wc["prim"] >= 0, wa["prim"] >= 0), (tier, group)
        assert not wa["t"].any() and not wa["point"].any()


# -------------------------------------------------------------- non-vacuity
def _f32_dir(rays):
    with np.errstate(all="ignore"):
        return q._ray_new_direction(rays["direction"])


@functools.lru_cache(maxsize=None)
def census():
    """The categories the bank exists for, counted from the oracle's answers and from quantities
    recomputed in f32 as the reference computes them."""
    c = {}
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]  # noqa: E731
    # sphere: tangent rays, disc == 0 (primitives.rs:57-81 with centre 0, radius 1)
    _, _, rays, _, _ = eb.case("lattice", "sphere/identity")
    want = eb.want_closest("lattice", "sphere/identity")
    d, oc = _f32_dir(rays), rays["origin"]
    hb, a, cc = dot(oc, d), dot(d, d), dot(oc, oc) - F(1) * F(1)
    disc = hb * hb - a * cc
    c["tangent disc == 0"] = int(((disc == 0) & (want["prim"] >= 0)).sum())
    # cube: a direction component below 1e-6 with the origin outside that slab (primitives.rs:301-364)
    _, _, rays, _, _ = eb.case("lattice", "cube/identity")
    want = eb.want_closest("lattice", "cube/identity")
    d, o = _f32_dir(rays), rays["origin"]
    par = ((np.abs(d) < F(1e-6)) & ((o < -1) | (o > 1))).any(1)
    assert not (par & (want["prim"] >= 0)).any()
    c["parallel-rejected"] = int(par.sum())
    inside = (np.abs(o) < 1).all(1)
    nf_normal = ~np.isfinite(want["normal"]).all(1) & (want["prim"] >= 0)
    c["origin inside, non-finite normal"] = int((inside & nf_normal).sum())
    # cone: hits at the apex (0, 1, 0) whose normal is 0/0
    want = eb.want_closest("lattice", "cone/identity")
    apex = (want["prim"] >= 0) & (want["point"] == np.array([0, 1, 0], F)).all(1)
    c["apex, non-finite normal"] = int((apex & ~np.isfinite(want["normal"]).all(1)).sum())
    # triangle: barycentrics of the hits, Moller-Trumbore as primitives.rs:208-244
    _, _, rays, _, _ = eb.case("lattice", "triangle/identity")
    want = eb.want_closest("lattice", "triangle/identity")
    hit = want["prim"] >= 0
    d, o = _f32_dir(rays)[hit], rays["origin"][hit]
    v0, v1, v2 = (np.array(v, F) for v in eb.TRI)
    e1, e2 = np.broadcast_to(v1 - v0, d.shape), np.broadcast_to(v2 - v0, d.shape)
    cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0],  # noqa: E731
                                   a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], 1)
    h = cross(d, e2)
    f = F(1) / dot(e1, h)
    s = o - v0
    u = f * dot(s, h)
    v = f * dot(d, cross(s, e1))
    c["triangle edge u == 0"] = int((u == 0).sum())
    c["triangle edge v == 0"] = int((v == 0).sum())
    c["triangle edge u + v == 1"] = int((u + v == 1).sum())
    # ties: both objects alone report the same t, and the pair's winner is index 0
    ties = 0
    for group in ("cube_plane", "plane_cube", "sphere_sdf", "sdf_sphere", "sphere_twice"):
        objs, lights, rays, _, _ = eb.case("ties", group)
        both = eb.want_closest("ties", group)
        alone = [q.oracle_closest(LoweredScene([ob], lights, Camera()), rays) for ob in objs[:2]]
        tie = (alone[0]["prim"] >= 0) & (alone[1]["prim"] >= 0) & \
              (alone[0]["t"].view(np.uint32) == alone[1]["t"].view(np.uint32))
        assert tie.sum() > 0, group
        assert (both["prim"][tie] == 0).all(), group
        ties += int(tie.sum())
    c["exact tie won by the lower index"] = ties
    # a mesh whose triangles are listed twice: the lower of the pair wins (the triangle-by-triangle form)
    w = eb.want_closest("ties", "dup_mesh_triangles")
    assert (w["prim"][w["prim"] >= 0] % 2 == 0).all()
    c["duplicate triangle won by the lower index"] = int((w["prim"] >= 0).sum())
    nan_t = inf_t = 0
    for group in eb.TIERS["scales"][1]:
        w = eb.want_closest("scales", group)
        nan_t += int(((w["prim"] >= 0) & np.isnan(w["t"])).sum())
        inf_t += int(((w["prim"] >= 0) & np.isinf(w["t"])).sum())
    c["NaN-t hit"], c["inf-t hit"] = nan_t, inf_t
    return c


def test_bank_is_not_vacuous():
    for kind in eb.ANALYTIC:
        w = eb.want_closest("lattice", f"{kind}/identity")
        hits = int((w["prim"] >= 0).sum())
        print(f"lattice {kind}: hits {hits} misses {len(w) - hits} of {len(w)}")
        assert len(w) == 8918 and hits >= 100 and len(w) - hits >= 100
    c = census()
    for k, v in c.items():
        print(f"{k}: {v}")
    assert all(v >= 1 for v in c.values()), c


def test_the_confirmed_divergence_is_in_the_bank():
    """(3e19, 0, 0) -> (1, 0, 0) against the unit sphere: the reference reports a hit with t = NaN
    (hb*hb and a*cc both overflow, disc = NaN, every comparison fails); at 3e18 it reports a miss."""
    _, _, rays, labels, _ = eb.case("scales", "far/sphere")
    w, wa = eb.want_closest("scales", "far/sphere"), eb.want_any("scales", "far/sphere")
    k = [i for i in range(len(rays)) if tuple(rays[i]["origin"]) == (F(3e19), 0, 0) and tuple(rays[i]["direction"]) == (1, 0, 0)]
    assert len(k) == 1 and labels[k[0]] == "scales/far/sphere/away/3e+19"
    assert w["prim"][k[0]] == 0 and np.isnan(w["t"][k[0]]) and wa["prim"][k[0]] == 0
    k = [i for i in range(len(rays)) if tuple(rays[i]["origin"]) == (F(3e18), 0, 0) and tuple(rays[i]["direction"]) == (1, 0, 0)]
    assert len(k) == 1 and w["prim"][k[0]] == -1 and wa["prim"][k[0]] == -1
