"""The edge-case ray bank: small scenes and RAY_DTYPE ray arrays aimed at the places where the
intersectors branch and where the proofs of the device's shortcuts state preconditions -- tangents
(disc == 0), rays parallel to faces, apexes, triangle edges (u == 0, v == 0, u + v == 1), exact ties
between objects, intervals that end on a hit, degenerate rays and objects, and the magnitudes at
which f32 squares overflow or go denormal.  CPU only and deterministic; nothing here touches the
device.  tests/test_edge_bank_cpu.py checks the checker on it (C oracle against the numpy
restatement), tests/test_gpu_edge_bank.py runs the device's queries over it.

Every tier is a function `tier(group) -> (objects, lights, rays, labels)`; TIERS lists the tiers in
the order they are meant to run and the groups of each.  `labels` names each ray's category."""
import functools

import numpy as np

import instance_ref
import query_ref as q
from rrte_amd import (Camera, Capsule, Color, Cone, Cube, Cylinder, LambertianMaterial, LoweredScene, Mesh, MeshInstance,
                      Plane, SDFBox, SDFCapsule, SDFCone, SDFCylinder, SDFEllipsoid, SDFObject, SDFPrism, SDFRing,
                      SDFSphere, SDFTorus, SDFTube, Sphere, Transform, Triangle, abi)
from rrte_amd.mesh import icosphere

F = np.float32
MAT = LambertianMaterial(Color.rgb(0.7, 0.5, 0.3))
MAT2 = LambertianMaterial(Color.rgb(0.2, 0.4, 0.6))
ANALYTIC = ["sphere", "plane", "cube", "cylinder", "cone", "capsule", "triangle"]
SDF_LEAVES = ["sdf_sphere", "sdf_box", "sdf_cylinder", "sdf_prism", "sdf_torus", "sdf_tube", "sdf_ring", "sdf_cone",
              "sdf_capsule", "sdf_ellipsoid"]
PLACEMENTS = ["identity", "exact", "rotated"]
# exact: translation by lattice values, scale by powers of two, mirrored in x, non-uniform (2, 0.5, 1)
EXACT = Transform(position=(0.5, -1.0, 1.0), scale=(-2.0, 0.5, 1.0))
# inexact: a rotation by 0.7 rad about (1, 2, 3) / sqrt(14)
_AX = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
ROTATED = Transform(rotation=(*(_AX * np.sin(0.35)), np.cos(0.35)))
SCALES = [-70, -62, -40, 40, 62, 64]  # squares overflow from 2^64 and go denormal from 2^-63


# ------------------------------------------------------------------ rays
@functools.lru_cache(maxsize=None)
def lattice():
    """Origins {-2,-1,-0.5,0,0.5,1,2}^3 times the 26 directions of {-1,0,1}^3 without 0: 8918 rays."""
    v = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], dtype=F)
    o = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    s = np.array([-1.0, 0.0, 1.0], dtype=F)
    d = np.stack(np.meshgrid(s, s, s, indexing="ij"), -1).reshape(-1, 3)
    d = d[np.abs(d).sum(1) > 0]
    oo, dd = np.repeat(o, len(d), axis=0), np.tile(d, (len(o), 1))
    oo.setflags(write=False)
    dd.setflags(write=False)
    return oo, dd


def subsample(n, m):
    """At most m of range(n), evenly strided from 0 (deterministic)."""
    if n <= m:
        return np.arange(n)
    return (np.arange(m, dtype=np.int64) * n) // m


def lattice_rays(m=None, t_min=q.T_MIN, t_max=q.INF):
    o, d = lattice()
    k = subsample(len(o), m or len(o))
    return q.rays_of(o[k], d[k], t_min, t_max)


def _labels(n, text):
    return np.full(n, text, dtype=object)


# ---------------------------------------------------------------- objects
def _map(tr, p):
    """p through a Transform in float64 (scale, rotate, translate), rounded to f32."""
    x, y, z, w = (float(v) for v in tr.rotation)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    s = np.array([float(v) for v in tr.scale])
    return tuple(F(v) for v in R @ (np.asarray(p, dtype=np.float64) * s) + np.array([float(v) for v in tr.position]))


TRI = [(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (-1.0, 1.0, 0.0)]  # edges x = -1 (u = 0), y = -1 (v = 0), x + y = 0


def analytic(kind, placement="identity", s=1.0):
    """One analytic object of `kind`, unit-ish at the origin and scaled by s, its surfaces on the
    lattice: sphere and cylinder radius 1 (tangent to the lines |x| = 1), cylinder and cone caps at
    |y| = 1 = hh, the cone's apex at (0, 1, 0) and rim at y = -1, the capsule's seam at y = 0, the
    cube's faces, edges and corners at +/-1, the triangle's edges and vertices on lattice points.
    Spheres, planes and triangles take no transform in the reference: their placement moves their
    own parameters."""
    tr = {"identity": Transform.identity(), "exact": EXACT, "rotated": ROTATED}[placement]
    if kind == "sphere":
        o = Sphere({"identity": (0, 0, 0), "exact": (0.5, -1.0, 1.0), "rotated": (0.3, 0.1, -0.2)}[placement],
                   {"identity": 1.0, "exact": 2.0, "rotated": 1.1}[placement] * s, MAT)
        o.center = tuple(F(c) * F(s) for c in o.center)
        return o
    if kind == "plane":
        pt, n = {"identity": ((0, 0, 0), (0, 1, 0)), "exact": ((0, -0.5, 0), (0, 0, -1)),
                 "rotated": ((0.1, 0.2, 0.3), (1, 2, 3))}[placement]
        return Plane(tuple(F(c) * F(s) for c in pt), n, MAT)
    if kind == "triangle":
        return Triangle(*[tuple(F(c) * F(s) for c in _map(tr, v)) for v in TRI], MAT)
    if kind == "cube":
        o = Cube((0, 0, 0), (2 * s, 2 * s, 2 * s), MAT)
    elif kind == "cylinder":
        o = Cylinder((0, 0, 0), 1.0 * s, 2.0 * s, MAT)
    elif kind == "cone":
        o = Cone((0, 0, 0), 1.0 * s, 2.0 * s, MAT)
    elif kind == "capsule":
        o = Capsule((0, 0, 0), 0.5 * s, 1.0 * s, MAT)
    else:
        raise KeyError(kind)
    o.set_transform(tr)
    return o


def sdf_leaf(kind, placement="identity", s=1.0):
    """One SDF leaf; SDF objects take no transform either: `exact` moves the centre by lattice values
    and doubles the sizes (no rotated placement)."""
    c = tuple(F(v) * F(s) for v in ((0, 0, 0) if placement == "identity" else (0.5, -1.0, 1.0)))
    k = (1.0 if placement == "identity" else 2.0) * s
    leaf = {"sdf_sphere": lambda: SDFSphere(c, 1.0 * k), "sdf_box": lambda: SDFBox(c, (2 * k, 2 * k, 2 * k)),
            "sdf_cylinder": lambda: SDFCylinder(c, 1.0 * k, 2.0 * k), "sdf_prism": lambda: SDFPrism(c, (2 * k, 2 * k, 2 * k)),
            "sdf_torus": lambda: SDFTorus(c, 1.0 * k, 0.5 * k), "sdf_tube": lambda: SDFTube(c, 1.0 * k, 0.5 * k, 2.0 * k),
            "sdf_ring": lambda: SDFRing(c, 1.0 * k, 0.5 * k), "sdf_cone": lambda: SDFCone(c, 1.0 * k, 2.0 * k),
            "sdf_capsule": lambda: SDFCapsule(c, 0.5 * k, 1.0 * k),
            "sdf_ellipsoid": lambda: SDFEllipsoid(c, (1.0 * k, 0.5 * k, 2.0 * k))}[kind]()
    return SDFObject(leaf, MAT)


def ico(s=1.0):
    m = icosphere((0, 0, 0), 1.0, 1, MAT)
    if s != 1.0:
        m = Mesh(m.positions * F(s), m.indices, m.normals, MAT, "icosphere")
    return m


def quad_mesh(dup=True):
    """A 2x2 grid of unit quads in the plane z = 0 over [-1, 1]^2 (8 triangles whose shared edges and
    vertices are lattice points), every triangle listed twice when dup."""
    xs = [-1.0, 0.0, 1.0]
    pos = np.array([(x, y, 0.0) for y in xs for x in xs], dtype=F)
    tri = []
    for j in range(2):
        for i in range(2):
            a, b, c, d = j * 3 + i, j * 3 + i + 1, (j + 1) * 3 + i, (j + 1) * 3 + i + 1
            tri += [(a, b, c), (b, d, c)]
    idx = np.array([t for t in tri for _ in range(2 if dup else 1)], dtype=np.uint32)
    return Mesh(pos, idx, np.tile(np.array([0, 0, 1], dtype=F), (len(pos), 1)), MAT, "quads")


def one_object(name, placement="identity", s=1.0):
    if name in ANALYTIC:
        return [analytic(name, placement, s)]
    if name in SDF_LEAVES:
        return [sdf_leaf(name, placement, s)]
    if name == "mesh":
        return [ico(s)]
    if name == "mesh_leaf":  # three triangles: the whole BVH is one leaf
        m = quad_mesh(dup=False)
        return [Mesh(m.positions * F(s), m.indices[[3, 0, 5]], m.normals, MAT, "leaf")]
    if name == "mesh_instance":  # the instance alone: its mesh is in the scene only through it
        return [MeshInstance(ico(s), {"identity": Transform.identity(), "exact": EXACT, "rotated": ROTATED}[placement], MAT)]
    raise KeyError(name)


# ------------------------------------------------------------------ tiers
def lattice_groups():
    g = [f"{k}/{p}" for k in ANALYTIC for p in PLACEMENTS]
    g += [f"{k}/{p}" for k in SDF_LEAVES for p in ("identity", "exact")]
    g += ["mesh/identity"] + [f"mesh_instance/{p}" for p in PLACEMENTS]
    return g


def tier_lattice(group):
    """The lattice bank against one object.  Analytic kinds at the identity get all 8918 rays, every
    other group an even sub-sample of 2048 (SDF marches and the transformed copies cost the checker's
    Python loop more)."""
    name, placement = group.split("/")
    full = name in ANALYTIC and placement == "identity"
    rays = lattice_rays(None if full else 2048)
    return one_object(name, placement), [], rays, _labels(len(rays), f"lattice/{group}")


INTERVAL_OBJECTS = ANALYTIC + SDF_LEAVES + ["mesh", "mesh_instance"]
INTERVALS = ["t_min=t", "t_max=t", "t_min=next(t)", "t_max=prev(t)", "t_max<t_min", "t_min=0", "t_max=nan", "t_min=nan"]


@functools.lru_cache(maxsize=None)
def lattice_want(group):
    objs, lights, rays, _ = tier_lattice(group)
    w = checker_closest(LoweredScene(objs, lights, _camera()), rays)
    w.setflags(write=False)
    return w


def has_instance(sc):
    return any(sc.prims[i].kind == abi.PRIM_MESH_INSTANCE for i in range(sc.ir.num_prims))


def checker_closest(sc, rays):
    """query_ref.oracle_closest; a scene with a mesh instance goes through instance_ref.closest (the
    C oracle has no instance kind), which also fills `tri`."""
    return instance_ref.closest(sc, rays) if has_instance(sc) else q.oracle_closest(sc, rays)


def checker_any(sc, rays):
    return instance_ref.any_hit(sc, rays) if has_instance(sc) else q.oracle_any(sc, rays)


def _camera():
    return Camera()


def tier_interval(name):
    """128 lattice rays with a finite hit t on the object, each cast again with the eight intervals of
    INTERVALS built from that t."""
    group = f"{name}/identity"
    objs, lights, rays, _ = tier_lattice(group)
    want = lattice_want(group)
    ok = np.flatnonzero((want["prim"] >= 0) & np.isfinite(want["t"]))
    ok = ok[subsample(len(ok), 128)]
    base, t = rays[ok], want["t"][ok].astype(F)
    out, labels = [], []
    nan = F(np.nan)
    for what in INTERVALS:
        r = base.copy()
        if what == "t_min=t":
            r["t_min"] = t
        elif what == "t_max=t":
            r["t_max"] = t
        elif what == "t_min=next(t)":
            r["t_min"] = np.nextafter(t, F(np.inf))
        elif what == "t_max=prev(t)":
            r["t_max"] = np.nextafter(t, F(-np.inf))
        elif what == "t_max<t_min":
            r["t_min"], r["t_max"] = t, t * F(0.5)
        elif what == "t_min=0":
            r["t_min"] = F(0)
        elif what == "t_max=nan":
            r["t_max"] = nan
        elif what == "t_min=nan":
            r["t_min"] = nan
        out.append(r)
        labels.append(_labels(len(r), f"interval/{name}/{what}"))
    return objs, lights, np.concatenate(out), np.concatenate(labels)


TIE_GROUPS = ["sphere_twice", "cube_twice", "sphere_sdf", "sdf_sphere", "cube_plane", "plane_cube", "coplanar_triangles",
              "dup_mesh", "dup_mesh_triangles"]


def tier_ties(group):
    """Exact ties: the reference takes objects in list order with a strict '<', so the lower index
    wins, and within a mesh the lowest triangle index.  `sphere_sdf` / `sdf_sphere` are a Sphere and a
    coincident SDFSphere in both orders, cast with t_min = the sphere's own hit t, so that the march
    starts and ends on min(t_max, best.t) and the SDF hit has exactly the analytic hit's t."""
    rays = lattice_rays(2048)
    if group == "sphere_twice":
        objs = [analytic("sphere"), analytic("sphere")]
    elif group == "cube_twice":
        objs = [analytic("cube"), analytic("cube")]
    elif group in ("sphere_sdf", "sdf_sphere"):
        objs = [analytic("sphere"), sdf_leaf("sdf_sphere")]
        rays = lattice_rays()
        want = lattice_want("sphere/identity")
        ok = np.flatnonzero((want["prim"] >= 0) & np.isfinite(want["t"]))
        ok = ok[subsample(len(ok), 512)]
        at_t = rays[ok].copy()
        at_t["t_min"] = want["t"][ok]
        rays = np.concatenate([at_t, rays[ok]])
        if group == "sdf_sphere":
            objs = objs[::-1]
    elif group in ("cube_plane", "plane_cube"):  # the cube's top face lies in the plane y = 1
        objs = [analytic("cube"), Plane((0, 1, 0), (0, 1, 0), MAT2)]
        if group == "plane_cube":
            objs = objs[::-1]
    elif group == "coplanar_triangles":
        objs = [analytic("triangle"), Triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), MAT2),
                Triangle((1, 1, 0), (-1, 1, 0), (-1, -1, 0), MAT)]
    elif group == "dup_mesh":
        objs = [quad_mesh()]
    elif group == "dup_mesh_triangles":
        objs = quad_mesh().triangles()
    else:
        raise KeyError(group)
    for o in objs[1:]:  # distinct materials name the winner in the record as well
        if o.material is MAT and objs[0].material is MAT:
            o.material = MAT2
    return objs, [], rays, _labels(len(rays), f"ties/{group}")


DEGENERATE_RAY_KINDS = ANALYTIC + SDF_LEAVES + ["mesh", "mesh_instance"]


@functools.lru_cache(maxsize=None)
def degenerate_rays():
    """64 rays: zero, negative-zero, denormal, infinite and NaN directions, and non-finite origins."""
    inf, nan, den = np.inf, np.nan, 1e-40
    dirs = [("zero", (0, 0, 0)), ("negzero", (-0.0, -0.0, -0.0)), ("negzero_z", (-0.0, -0.0, -1.0)),
            ("negzero_y", (0.0, 1.0, -0.0)), ("denormal_x", (den, 0, 0)), ("denormal_xyz", (den, -den, den)),
            ("denormal_mixed", (den, 0, -1.0)), ("inf_x", (inf, 0, 0)), ("neginf_y", (0, -inf, 0)),
            ("inf_xyz", (inf, inf, inf)), ("inf_mixed", (1.0, inf, 0)), ("nan_x", (nan, 0, 0)),
            ("nan_mixed", (1.0, nan, 0)), ("nan_z", (0, 0, nan)), ("huge", (3e38, 3e38, 0)), ("tiny", (1e-30, 0, 1e-30))]
    origins = [(0, 0, 0), (2, 0.5, 0), (0, 2, 0)]
    o, d, lab = [], [], []
    for name, dv in dirs:
        for ov in origins:
            o.append(ov), d.append(dv), lab.append(f"direction/{name}")
    bad_o = [("inf_x", (inf, 0, 0)), ("neginf_y", (0, -inf, 0)), ("nan_x", (nan, 0, 0)), ("nan_z", (0, 0, nan)),
             ("inf_xyz", (inf, -inf, inf)), ("huge", (3e38, 0, 0)), ("nan_all", (nan, nan, nan)), ("inf_z", (0, 0, inf))]
    for name, ov in bad_o:
        for dv in [(0, 0, -1), (-1, 0, 0)]:
            o.append(ov), d.append(dv), lab.append(f"origin/{name}")
    assert len(o) == 64
    with np.errstate(over="ignore"):
        return np.array(o, dtype=F), np.array(d, dtype=F), np.array(lab, dtype=object)


def tier_degenerate_rays(name):
    o, d, lab = degenerate_rays()
    return one_object(name), [], q.rays_of(o, d), np.array([f"degenerate_ray/{name}/{s}" for s in lab], dtype=object)


def _tri(v0, v1, v2):
    with np.errstate(all="ignore"):
        return Triangle(v0, v1, v2, MAT)


def _xf(o, tr):
    o.set_transform(tr)
    return o


DEGENERATE_OBJECTS = {
    "sphere_r0": lambda: [Sphere((0, 0, 0), 0.0, MAT)],
    "sphere_negative_r": lambda: [Sphere((0, 0, 0), -1.0, MAT)],
    "cube_flat": lambda: [Cube((0, 0, 0), (2, 0, 2), MAT)],
    "cylinder_r0": lambda: [Cylinder((0, 0, 0), 0.0, 2.0, MAT)],
    "cylinder_h0": lambda: [Cylinder((0, 0, 0), 1.0, 0.0, MAT)],
    "cone_r0": lambda: [Cone((0, 0, 0), 0.0, 2.0, MAT)],
    "cone_h0": lambda: [Cone((0, 0, 0), 1.0, 0.0, MAT)],
    "triangle_point": lambda: [_tri((0, 0, 0), (0, 0, 0), (0, 0, 0))],
    "triangle_collinear": lambda: [_tri((-1, 0, 0), (0, 0, 0), (1, 0, 0))],
    "plane_zero_normal": lambda: [_plane_zero()],
    "cube_scale0": lambda: [_xf(Cube((0, 0, 0), (2, 2, 2), MAT), Transform(scale=(1.0, 0.0, 1.0)))],
    "cylinder_scale0": lambda: [_xf(Cylinder((0, 0, 0), 1.0, 2.0, MAT), Transform(scale=(0.0, 1.0, 1.0)))],
    "mesh_one_triangle": lambda: [Mesh(np.array(TRI, dtype=F), [[0, 1, 2]], None, MAT)],
}
# rejected by validate_scene (RRTE_INVALID_ARG, nothing written)
REJECTED_OBJECTS = {
    "mesh_instance_scale0": lambda: [MeshInstance(ico(), Transform(scale=(1.0, 0.0, 1.0)), MAT)],
}


def _plane_zero():
    with np.errstate(all="ignore"):
        return Plane((0, 0, 0), (0, 0, 0), MAT)


def tier_degenerate_objects(group):
    rays = lattice_rays(1024)
    objs = (DEGENERATE_OBJECTS.get(group) or REJECTED_OBJECTS[group])()
    return objs, [], rays, _labels(len(rays), f"degenerate_object/{group}")


SCALE_OBJECTS = ["sphere", "cube", "cylinder", "triangle", "sdf_sphere", "mesh", "mesh_leaf"]
FAR_K = [40, 62, 64]
# far from the object in its own units, yet nowhere near an overflow; a mesh is scanned in its original
# order from 2^24 of its extents (~2) on: 2^24 is the last distance whose rays still walk the BVH
MID_K = [10, 20, 24, 26, 30]


def tier_scales(group):
    """`<object>/<k>`: object and lattice rays (1024 of them) scaled together by 2^k, t_min = 2^(k-10).
    `far/<object>`: the unscaled object with origins 2^k and 3e19 away along each axis and two
    diagonals, moving towards and away (the case (3e19, 0, 0) -> (1, 0, 0) is one of them).
    `mid/<object>`: the same from 2^k away, k in MID_K."""
    a, b = group.split("/")
    if a in ("far", "mid"):
        dist = [F(2.0) ** F(k) for k in FAR_K] + [F(3e19), F(3e18)] if a == "far" else [F(2.0) ** F(k) for k in MID_K]
        axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (-1, 1, 1)]
        o, d, lab = [], [], []
        for r in dist:
            for ax in axes:
                for sgn, way in ((1.0, "away"), (-1.0, "towards")):
                    for off in ((0, 0, 0), (0.5, 0.5, 0.5)):  # through the centre, and off the lattice
                        o.append([F(c) * r + F(f) for c, f in zip(ax, off)])
                        d.append([F(c) * F(sgn) for c in ax])
                        lab.append(f"scales/{a}/{b}/{way}/{float(r):.3g}")
        with np.errstate(over="ignore"):
            rays = q.rays_of(np.array(o, dtype=F), np.array(d, dtype=F))
        return one_object(b), [], rays, np.array(lab, dtype=object)
    k = int(b)
    s = float(2.0 ** k)
    o, d = lattice()
    pick = subsample(len(o), 1024)
    rays = q.rays_of(o[pick] * F(s), d[pick], F(2.0 ** (k - 10)), q.INF)
    return one_object(a, "identity", s), [], rays, _labels(len(rays), f"scales/{group}")


def scale_groups():
    return [f"{o}/{k}" for o in SCALE_OBJECTS for k in SCALES] + [f"{a}/{o}" for a in ("far", "mid") for o in SCALE_OBJECTS]


# in the order the device runs them: the two degenerate tiers last
TIERS = {
    "lattice": (tier_lattice, lattice_groups()),
    "interval": (tier_interval, INTERVAL_OBJECTS),
    "ties": (tier_ties, TIE_GROUPS),
    "scales": (tier_scales, scale_groups()),
    "degenerate_rays": (tier_degenerate_rays, DEGENERATE_RAY_KINDS),
    "degenerate_objects": (tier_degenerate_objects, list(DEGENERATE_OBJECTS)),
}
CASES = [(t, g) for t, (_, groups) in TIERS.items() for g in groups]


@functools.lru_cache(maxsize=None)
def case(tier, group):
    """(objects, lights, rays, labels, lowered scene) of one case; built once, rays read-only."""
    with np.errstate(all="ignore"):  # (degenerate and huge objects: the constructors normalise in f32)
        objs, lights, rays, labels = TIERS[tier][0](group)
    rays.setflags(write=False)
    return objs, lights, rays, labels, LoweredScene(objs, lights, _camera())


@functools.lru_cache(maxsize=None)
def want_closest(tier, group):
    *_, rays, _, sc = case(tier, group)
    w = checker_closest(sc, rays)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def want_any(tier, group):
    *_, rays, _, sc = case(tier, group)
    w = checker_any(sc, rays)
    w.setflags(write=False)
    return w


def non_finite(hits):
    """Hits with a non-finite t, point or normal."""
    hit = hits["prim"] >= 0
    return hit & ~(np.isfinite(hits["t"]) & np.isfinite(hits["point"]).all(1) & np.isfinite(hits["normal"]).all(1))


def describe(tier, group, bad):
    """The labels and rays of the failing indices `bad`, for an assertion message."""
    _, _, rays, labels, _ = case(tier, group)
    return [(str(labels[i]), rays[i]) for i in list(bad)[:5]]


# Hits with a non-finite t, point or normal in the oracle's closest-hit answers, per case: established
# on the CPU (tests/test_edge_bank_cpu.py asserts them) and asserted again where the device runs, in
# place of the random-ray tests' cap on non-finite records.
NON_FINITE = {
    ('lattice', 'sphere/identity'): 0,
    ('lattice', 'sphere/exact'): 0,
    ('lattice', 'sphere/rotated'): 0,
    ('lattice', 'plane/identity'): 0,
    ('lattice', 'plane/exact'): 0,
    ('lattice', 'plane/rotated'): 0,
    ('lattice', 'cube/identity'): 2072,
    ('lattice', 'cube/exact'): 200,
    ('lattice', 'cube/rotated'): 389,
    ('lattice', 'cylinder/identity'): 0,
    ('lattice', 'cylinder/exact'): 0,
    ('lattice', 'cylinder/rotated'): 0,
    ('lattice', 'cone/identity'): 30,
    ('lattice', 'cone/exact'): 10,
    ('lattice', 'cone/rotated'): 0,
    ('lattice', 'capsule/identity'): 0,
    ('lattice', 'capsule/exact'): 0,
    ('lattice', 'capsule/rotated'): 0,
    ('lattice', 'triangle/identity'): 0,
    ('lattice', 'triangle/exact'): 0,
    ('lattice', 'triangle/rotated'): 0,
    ('lattice', 'sdf_sphere/identity'): 0,
    ('lattice', 'sdf_sphere/exact'): 0,
    ('lattice', 'sdf_box/identity'): 2,
    ('lattice', 'sdf_box/exact'): 2,
    ('lattice', 'sdf_cylinder/identity'): 0,
    ('lattice', 'sdf_cylinder/exact'): 0,
    ('lattice', 'sdf_prism/identity'): 0,
    ('lattice', 'sdf_prism/exact'): 0,
    ('lattice', 'sdf_torus/identity'): 0,
    ('lattice', 'sdf_torus/exact'): 0,
    ('lattice', 'sdf_tube/identity'): 0,
    ('lattice', 'sdf_tube/exact'): 0,
    ('lattice', 'sdf_ring/identity'): 0,
    ('lattice', 'sdf_ring/exact'): 0,
    ('lattice', 'sdf_cone/identity'): 0,
    ('lattice', 'sdf_cone/exact'): 0,
    ('lattice', 'sdf_capsule/identity'): 0,
    ('lattice', 'sdf_capsule/exact'): 0,
    ('lattice', 'sdf_ellipsoid/identity'): 0,
    ('lattice', 'sdf_ellipsoid/exact'): 0,
    ('lattice', 'mesh/identity'): 0,
    ('lattice', 'mesh_instance/identity'): 0,
    ('lattice', 'mesh_instance/exact'): 0,
    ('lattice', 'mesh_instance/rotated'): 0,
    ('interval', 'sphere'): 0,
    ('interval', 'plane'): 0,
    ('interval', 'cube'): 635,
    ('interval', 'cylinder'): 0,
    ('interval', 'cone'): 6,
    ('interval', 'capsule'): 0,
    ('interval', 'triangle'): 0,
    ('interval', 'sdf_sphere'): 3,
    ('interval', 'sdf_box'): 6,
    ('interval', 'sdf_cylinder'): 1,
    ('interval', 'sdf_prism'): 0,
    ('interval', 'sdf_torus'): 0,
    ('interval', 'sdf_tube'): 0,
    ('interval', 'sdf_ring'): 0,
    ('interval', 'sdf_cone'): 0,
    ('interval', 'sdf_capsule'): 5,
    ('interval', 'sdf_ellipsoid'): 3,
    ('interval', 'mesh'): 0,
    ('interval', 'mesh_instance'): 0,
    ('ties', 'sphere_twice'): 0,
    ('ties', 'cube_twice'): 467,
    ('ties', 'sphere_sdf'): 0,
    ('ties', 'sdf_sphere'): 0,
    ('ties', 'cube_plane'): 467,
    ('ties', 'plane_cube'): 467,
    ('ties', 'coplanar_triangles'): 0,
    ('ties', 'dup_mesh'): 0,
    ('ties', 'dup_mesh_triangles'): 0,
    ('scales', 'sphere/-70'): 0,
    ('scales', 'sphere/-62'): 0,
    ('scales', 'sphere/-40'): 0,
    ('scales', 'sphere/40'): 0,
    ('scales', 'sphere/62'): 0,
    ('scales', 'sphere/64'): 1024,
    ('scales', 'cube/-70'): 239,
    ('scales', 'cube/-62'): 239,
    ('scales', 'cube/-40'): 239,
    ('scales', 'cube/40'): 239,
    ('scales', 'cube/62'): 239,
    ('scales', 'cube/64'): 239,
    ('scales', 'cylinder/-70'): 0,
    ('scales', 'cylinder/-62'): 0,
    ('scales', 'cylinder/-40'): 0,
    ('scales', 'cylinder/40'): 0,
    ('scales', 'cylinder/62'): 0,
    ('scales', 'cylinder/64'): 0,
    ('scales', 'triangle/-70'): 0,
    ('scales', 'triangle/-62'): 0,
    ('scales', 'triangle/-40'): 0,
    ('scales', 'triangle/40'): 53,
    ('scales', 'triangle/62'): 53,
    ('scales', 'triangle/64'): 692,
    ('scales', 'sdf_sphere/-70'): 165,
    ('scales', 'sdf_sphere/-62'): 153,
    ('scales', 'sdf_sphere/-40'): 153,
    ('scales', 'sdf_sphere/40'): 157,
    ('scales', 'sdf_sphere/62'): 157,
    ('scales', 'sdf_sphere/64'): 83,
    ('scales', 'mesh/-70'): 0,
    ('scales', 'mesh/-62'): 0,
    ('scales', 'mesh/-40'): 0,
    ('scales', 'mesh/40'): 0,
    ('scales', 'mesh/62'): 227,
    ('scales', 'mesh/64'): 441,
    ('scales', 'mesh_leaf/-70'): 0,
    ('scales', 'mesh_leaf/-62'): 0,
    ('scales', 'mesh_leaf/-40'): 0,
    ('scales', 'mesh_leaf/40'): 0,
    ('scales', 'mesh_leaf/62'): 59,
    ('scales', 'mesh_leaf/64'): 266,
    ('scales', 'far/sphere'): 64,
    ('scales', 'far/cube'): 0,
    ('scales', 'far/cylinder'): 18,
    ('scales', 'far/triangle'): 0,
    ('scales', 'far/sdf_sphere'): 25,
    ('scales', 'far/mesh'): 0,
    ('scales', 'far/mesh_leaf'): 0,
    ('scales', 'mid/sphere'): 0,
    ('scales', 'mid/cube'): 0,
    ('scales', 'mid/cylinder'): 27,
    ('scales', 'mid/triangle'): 0,
    ('scales', 'mid/sdf_sphere'): 24,
    ('scales', 'mid/mesh'): 0,
    ('scales', 'mid/mesh_leaf'): 0,
    ('degenerate_rays', 'sphere'): 54,
    ('degenerate_rays', 'plane'): 36,
    ('degenerate_rays', 'cube'): 56,
    ('degenerate_rays', 'cylinder'): 0,
    ('degenerate_rays', 'cone'): 1,
    ('degenerate_rays', 'capsule'): 0,
    ('degenerate_rays', 'triangle'): 42,
    ('degenerate_rays', 'sdf_sphere'): 1,
    ('degenerate_rays', 'sdf_box'): 35,
    ('degenerate_rays', 'sdf_cylinder'): 43,
    ('degenerate_rays', 'sdf_prism'): 14,
    ('degenerate_rays', 'sdf_torus'): 0,
    ('degenerate_rays', 'sdf_tube'): 38,
    ('degenerate_rays', 'sdf_ring'): 0,
    ('degenerate_rays', 'sdf_cone'): 0,
    ('degenerate_rays', 'sdf_capsule'): 2,
    ('degenerate_rays', 'sdf_ellipsoid'): 40,
    ('degenerate_rays', 'mesh'): 50,
    ('degenerate_rays', 'mesh_instance'): 53,
    ('degenerate_objects', 'sphere_r0'): 8,
    ('degenerate_objects', 'sphere_negative_r'): 0,
    ('degenerate_objects', 'cube_flat'): 13,
    ('degenerate_objects', 'cylinder_r0'): 32,
    ('degenerate_objects', 'cylinder_h0'): 0,
    ('degenerate_objects', 'cone_r0'): 32,
    ('degenerate_objects', 'cone_h0'): 0,
    ('degenerate_objects', 'triangle_point'): 0,
    ('degenerate_objects', 'triangle_collinear'): 0,
    ('degenerate_objects', 'plane_zero_normal'): 1024,
    ('degenerate_objects', 'cube_scale0'): 1024,
    ('degenerate_objects', 'cylinder_scale0'): 0,
    ('degenerate_objects', 'mesh_one_triangle'): 0,
}
