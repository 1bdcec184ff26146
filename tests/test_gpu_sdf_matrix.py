"""The SDF path on the device over the catalogue of tests/sdf_matrix.py: every leaf, CSG op, deformer
axis combination (3 twist, 6 taper, 9 bend, 9 wave), noise at 1, 4 and RRTE_SDF_MAX_OCTAVES octaves,
a three-part chain and the point stack at RRTE_SDF_MAX_POINT_STACK.

1. Queries: the 1 024 rays of each case through Raytracer.raycast, closest and any-hit, bit for bit
   against the oracle loop (tests/query_ref.py), and the same records through the geometric check
   against the float64 reference (tests/sdf_f64.py) that tests/test_sdf_f64_cpu.py holds the oracle to.
2. Kernel variants: each case over a ground sphere under one point light, 35 x 19, REFCOMPAT depth 1
   and LAMBERT_SHADOW, by test_gpu_parity.compare's rule (linear image bit-exact, shadow-ray counts
   equal, the expected kernel active).  Single objects through the generic kernel; the matrix packed
   into scenes of at most nine objects through the generic, full and topology specialised kernels
   (where the axis indices are compile-time constants) and through the scene accelerator.
3. The shapes whose bounding sphere used to clip them, as queries: solid rays through the part that
   was clipped are hits.
"""
import functools

import numpy as np
import pytest

import oracle
import query_ref as q
import sdf_matrix as SM
from rrte_amd import Color, LambertianMaterial, LoweredScene, PointLight, Raytracer, RaytracerConfig, Sphere, abi, scenes
from test_gpu_refit import VARIANTS

pytestmark = pytest.mark.gpu

CASES = [pytest.param(c, id=c.name) for c in SM.CATALOGUE]
W, H = 35, 19
tolerance = SM.tolerance
MODES = ("refcompat", "lambert_shadow")


def raycast(case, any_hit):
    r = SM.rays(case)
    rt = Raytracer(device=0, jit=abi.JIT_OFF)
    return rt.raycast([SM.sdf_object(case)], r["origin"], r["direction"], t_min=SM.T_MIN, t_max=r["t_max"], any_hit=any_hit)


@functools.lru_cache(maxsize=None)
def oracle_any(case):
    return q.oracle_any(SM.lowered(case)[0], SM.rays(case))


# ---------------------------------------------------------------------------------- 1. queries
@pytest.mark.parametrize("case", CASES)
def test_queries(case):
    got = raycast(case, False)
    q.assert_hits_equal(got, SM.oracle_hits(case))
    SM.check_hits(case, got, tolerance(case))
    q.assert_hits_equal(raycast(case, True), oracle_any(case), tri=True)


# --------------------------------------------------------------------------- 2. kernel variants
GROUND_Y = -2.6   # below the lowest shape (taper-grow reaches 2.0 from its centre)
GROUPS = {
    "leaves-a": SM.LEAVES[:5], "leaves-b": SM.LEAVES[5:], "csg-sphere-box": SM.CSG[:6], "csg-ellipsoid-cylinder": SM.CSG[6:],
    "twist-taper-shrink": SM.TWIST + SM.TAPER[:3], "taper-grow": SM.TAPER[3:], "bend": SM.BEND, "wave": SM.WAVE, "noise-chain-nested": SM.NOISE + SM.COMPOSED,
}
assert sorted(c.name for g in GROUPS.values() for c in g) == sorted(SM.BY_NAME) and all(len(g) <= 9 for g in GROUPS.values())


def _materials():
    return [LambertianMaterial(Color.rgb(*c)) for c in [(0.8, 0.4, 0.3), (0.3, 0.7, 0.6), (0.6, 0.6, 0.9)]]


def _config(mode):
    return RaytracerConfig(max_depth=1, samples_per_pixel=1, width=W, height=H, mode=mode, jitter="center",
                           background_color=Color(0.05, 0.05, 0.08, 1.0))


def _ground():
    return Sphere((0.0, GROUND_Y - 1000.0, 0.0), 1000.0, LambertianMaterial(Color.rgb(0.3, 0.3, 0.3)))


def single_scene(case):
    """The case's object over a ground sphere under one point light, the camera at three times its reach."""
    reach = SM.region(case)[3]
    c = SM.anchor(case)
    eye = c + reach * np.array([1.6, 1.3, 2.4])
    objs = [_ground(), SM.sdf_object(case, _materials()[0])]
    lights = [PointLight(tuple(c + np.array([2.0, 6.0, 3.0])), Color.rgb(1, 1, 1), 40.0)]
    return objs, lights, scenes._camera(W, H, tuple(eye), tuple(c), 40.0)


def packed_scene(name):
    """A group's objects on a grid of three columns over the ground sphere under one point light; the grid's pitch
    keeps the widest shape of the group clear of its neighbours."""
    ms = _materials()
    objs = [_ground()]
    pitch = 2.0 * max(SM.region(c)[3] for c in GROUPS[name]) + 0.5
    rows = (len(GROUPS[name]) + 2) // 3
    for i, case in enumerate(GROUPS[name]):
        shift = ((i % 3 - 1) * pitch, 0.0, (i // 3 - 0.5 * (rows - 1)) * pitch)
        objs.append(SM.SDFObject(SM.build_at(case, shift), ms[i % 3], **{"max_steps": SM.MAX_STEPS, **case.object_args}))
    lights = [PointLight((1.2 * pitch, 4.0 * pitch, 2.5 * pitch), Color.rgb(1, 1, 1), 12.0 * pitch * pitch)]
    return objs, lights, scenes._camera(W, H, (0.25 * pitch, 1.5 * pitch, 1.8 * pitch), (0.0, -0.4, 0.0), 46.0)


_frames = {}


def oracle_frame(key, objs, lights, cam, mode):
    """(linear f32 image, shadow rays, pixels the SDF objects change) of a scene, once per key."""
    if (key, mode) not in _frames:
        prm = _config(mode).lower()
        _, lin, shadow = oracle.render(LoweredScene(objs, lights, cam), prm, nthreads=8, linear=True)
        _, bare, _ = oracle.render(LoweredScene(objs[:1], lights, cam), prm, nthreads=8, linear=True)
        shows = int((lin.view(np.uint32).reshape(-1, 4) != bare.view(np.uint32).reshape(-1, 4)).any(1).sum())
        lin.setflags(write=False)
        _frames[(key, mode)] = (lin, shadow, shows)
    return _frames[(key, mode)]


def check_frames(key, objs, lights, cam, min_shows, jit=abi.JIT_OFF, expect_jit=0, accel=False):
    for mode in MODES:
        want, shadow, shows = oracle_frame(key, objs, lights, cam, mode)
        assert shows >= min_shows, (key, mode, shows)
        kw = dict(scene_accel=abi.SCENE_ACCEL_ON, accel_min_prims=1) if accel else {}
        rt = Raytracer(_config(mode), device=0, jit=jit, **kw)
        _, got = rt.render_f32(objs, lights, [], cam, linear=True)
        st = rt.stats()
        assert st.jit_active == expect_jit, (key, mode, "unexpected kernel path", st.jit_active)
        if accel:
            a = rt.ctx.accel_info()
            # (four objects make one leaf and no inner node: the tree is built all the same)
            assert (a.builds, a.fallbacks, a.bounded) == (1, 0, len(objs)), (a.builds, a.fallbacks, a.bounded)
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(-1, 4).any(1))
        assert bad.size == 0, (key, mode, bad.size, bad[:8], got.reshape(-1, 4)[bad[:4]], want.reshape(-1, 4)[bad[:4]])
        assert int(st.shadow_rays) == shadow, (key, mode)
        assert st.primary_rays == W * H


@pytest.mark.parametrize("case", CASES)
def test_single_object_frames_generic(case):
    check_frames(case.name, *single_scene(case), min_shows=40)


@pytest.mark.parametrize("variant", list(VARIANTS) + ["accelerated"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_packed_frames(group, variant, monkeypatch):
    jit, topo, expect = VARIANTS.get(variant, (abi.JIT_OFF, None, 0))
    if topo is None:
        monkeypatch.delenv("RRTE_JIT_TOPO", raising=False)
    else:
        monkeypatch.setenv("RRTE_JIT_TOPO", topo)
    objs, lights, cam = packed_scene(group)
    check_frames(group, objs, lights, cam, min_shows=10 * (len(objs) - 1), jit=jit, expect_jit=expect,
                 accel=variant == "accelerated")


# ----------------------------------------------------------------------- 3. the bound cases
@pytest.mark.parametrize("name,clipped_before", [("inverted-capsule", 300), ("inverted-capsule-long", 200),
                                                 ("tapered-spheres", 40), ("thin-ellipsoids", 0)])
def test_formerly_clipped_shapes(name, clipped_before):
    """The shapes whose lowered sphere was too small (tests/test_sdf_f64_cpu.py bounds): the device
    agrees with the oracle bit for bit, and the solid rays whose first solid sample lies outside the old
    sphere -- where the march used to begin too late, or never -- are hits no later than that sample.

    thin-ellipsoids: the sliver the old sphere cut off (2.103 to 2.112) is thinner than any depth m
    the classification may use, so no solid ray passes through it, and the ellipsoid bound of radii
    (1.5, 0.1, 1.5) is no distance (its slope reaches r_max / r_min = 15), so a march at step scale 1
    may land inside: there only solid => hit and clear => miss are asserted."""
    case = SM.BOUND_BY_NAME[name]
    got = raycast(case, False)
    q.assert_hits_equal(got, SM.oracle_hits(case))
    kind, t_solid = SM.classified(case)
    was_clipped = SM.formerly_clipped(case)
    assert len(was_clipped) >= clipped_before, (name, len(was_clipped))
    hit = got["prim"] >= 0
    if name == "thin-ellipsoids":
        assert hit[kind == SM.sdf_f64.SOLID].all() and not hit[kind == SM.sdf_f64.CLEAR].any()
        assert (kind == SM.sdf_f64.SOLID).sum() >= 200 and (kind == SM.sdf_f64.CLEAR).sum() >= 200
    else:
        SM.check_hits(case, got, tolerance(case))
    assert hit[was_clipped].all() and (got["t"][was_clipped] <= t_solid[was_clipped]).all()


def test_mirrored_capsule_is_empty():
    """A capsule of negative radius holds no point; its sphere has a radius that is not negative."""
    case = SM.BOUND_BY_NAME["mirrored-capsule"]
    sc = SM.lowered(case)[0]
    assert sc.prims[0].p[3] >= 0.0
    rng = np.random.default_rng(5)
    o = (np.array(SM.anchor(case)) + 3.0 * SM._sphere_lattice(256, rng)).astype(np.float32)
    d = (np.array(SM.anchor(case)) + rng.uniform(-0.6, 0.6, (256, 3)) - o).astype(np.float32)
    got = Raytracer(device=0, jit=abi.JIT_OFF).raycast([SM.sdf_object(case)], o, d)
    q.assert_hits_equal(got, q.oracle_closest(sc, q.rays_of(o, d)))
    assert (got["prim"] < 0).all()
