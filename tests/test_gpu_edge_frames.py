"""Edge-case frames: the ray bank's placements (tests/edge_bank.py) seen through the frame kernels.
Queries only reach the runtime-scene kernel; the scene-specialised intersectors, the lane-parallel
shadow cull, the secant exits, the plain entry and the all-miss tiles are reached only by frames.

Two grid scenes -- every analytic kind (7 objects, 2 lights: the lane-parallel cull), and SDF leaves, a
two-leaf CSG and a small mesh -- rendered at 16x16 and 24x16 through an exact orthographic camera
along -z (every pixel ray exactly (0, 0, -1), origins on a 1/8 lattice: tangent rays, rays in cube
faces, through the cone's apex, on triangle edges), the same camera turned along -x, -y and +z by
look_at (inexact: origins an ulp off, a direction such as (0, -8.7e-08, 1) in the cube's "parallel"
branch), and a perspective camera with its eye inside the cube, at the sphere's centre and on the
plane.  Lights: a directional light exactly along an axis, a point light exactly on a surface point a
pixel hits (a zero-length shadow direction), a point light at a sphere's centre; no spot lights
(their acosf costs the linear image its exactness).

Each frame against oracle.render: the linear image bit for bit or NaN on both sides, the RGBA8
bytes within 1, identical shadow-ray counts, jit_active as requested -- in both modes, with the generic
kernel, the full and the topology specialised kernel, and RRTE_CULL and RRTE_TILE_CULL off and on."""
import functools
import itertools

import numpy as np
import pytest

import edge_bank as eb
import instance_ref
import oracle
from rrte_amd import (Camera, Capsule, Color, Cone, CSGComposite, Cube, Cylinder, DirectionalLight, LoweredScene,
                      MeshInstance, Plane, PointLight, Raytracer, RaytracerConfig, SDFBox, SDFObject, SDFSphere, Sphere,
                      Transform, Triangle, abi, to_radians, vec3)
from rrte_amd.mesh import Mesh

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (24, 16)]
WHITE = Color.rgb(1.0, 1.0, 1.0)


def analytic_grid():
    """Every analytic kind on the pixel lattice of the -z orthographic frame (pixel centres at odd
    multiples of 1/8): the sphere's silhouette, the cylinder's and the capsule's are tangent to pixel
    rays, the cube's faces contain pixel rays, one goes through the cone's apex and others along the
    triangle's edges.  7 objects x 2 lights <= 64: the lane-parallel shadow cull."""
    objs = [Sphere((-1.125, 1.125, 0.125), 0.5, eb.MAT), Cube((0.125, 1.125, 0.0), (0.5, 0.5, 0.5), eb.MAT2),
            Cylinder((1.125, 1.125, 0.0), 0.5, 0.5, eb.MAT), Cone((-1.125, -0.125, 0.0), 0.5, 0.5, eb.MAT2),
            Capsule((0.125, -0.125, 0.0), 0.25, 0.5, eb.MAT), Triangle((0.875, -0.375, 0.0), (1.375, -0.375, 0.0),
                                                                      (0.875, 0.125, 0.0), eb.MAT2),
            Plane((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), eb.MAT)]
    # the point light sits exactly on the sphere's point nearest the -z camera, which pixel (3, 3) hits
    lights = [DirectionalLight((0.0, 0.0, -1.0), WHITE, 0.8), PointLight((-1.125, 1.125, 0.625), WHITE, 1.5)]
    return objs, lights


def small_mesh():
    m = eb.ico()
    return Mesh(m.positions * np.float32(0.5) + np.array([1.125, -1.125, 0.0], np.float32), m.indices, m.normals, eb.MAT2)


def sdf_grid(instance=False):
    """SDF leaves, a two-leaf CSG, a small mesh (with `instance`, a mirrored copy of it too) and a
    sphere with a point light at its centre, over the same plane."""
    mesh = small_mesh()
    objs = [SDFObject(SDFSphere((-1.125, 1.125, 0.125), 0.5), eb.MAT), SDFObject(SDFBox((0.125, 1.125, 0.0), (0.5, 0.5, 0.5)), eb.MAT2),
            SDFObject(CSGComposite(SDFSphere((-1.125, -0.125, 0.0), 0.5), SDFBox((-0.875, -0.125, 0.0), (0.5, 0.25, 0.5)),
                                   "smooth_union", 0.125), eb.MAT),
            Sphere((0.125, -1.125, 0.0), 0.375, eb.MAT2), mesh, Plane((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), eb.MAT)]
    if instance:
        objs.insert(5, MeshInstance(mesh, Transform(position=(-2.5, 2.0, 0.0), scale=(-1.0, 0.5, 1.0)), eb.MAT))
    lights = [PointLight((0.125, -1.125, 0.0), WHITE, 1.5), PointLight((0.125, 0.125, 2.0), WHITE, 1.0)]
    if not instance:
        lights[1] = DirectionalLight((0.0, -1.0, 0.0), WHITE, 0.8)
    return objs, lights


SCENES = {"analytic": analytic_grid, "sdf": sdf_grid}


def cameras(w, h):
    out = {}
    for name, pos in (("ortho-z", (0, 0, 8)), ("ortho-x", (8, 0, 0)), ("ortho-y", (0, 8, 0)), ("ortho+z", (0, 0, -8))):
        cam = Camera.new_orthographic(-2.0, 2.0, -2.0, 2.0, 0.1, 100.0)
        cam.transform.position = vec3(*pos)
        if name != "ortho-z":  # (ortho-z keeps the identity rotation: exact)
            cam.look_at((0.0, 0.0, 0.0))
        out[name] = cam
    for name, pos in (("eye-in-cube", (0.125, 1.125, 0.0)), ("eye-at-sphere-centre", (-1.125, 1.125, 0.125)),
                      ("eye-on-plane", (0.5, 0.5, -1.0))):
        cam = Camera.new_perspective(to_radians(60.0), w / h, 0.1, 100.0)
        cam.transform.position = vec3(*pos)
        if name == "eye-on-plane":
            cam.look_at((0.0, 0.0, 1.0))
        out[name] = cam
    return out


CAMERAS = list(cameras(16, 16))


def config(w, h, mode):
    return RaytracerConfig(width=w, height=h, samples_per_pixel=1, max_depth=1, mode=mode, jitter="center")


@functools.lru_cache(maxsize=None)
def want(scene, mode, cam, w, h):
    objs, lights = SCENES[scene]()
    sc = LoweredScene(objs, lights, cameras(w, h)[cam])
    prm = config(w, h, mode).lower()
    r8, _, shadow = oracle.render(sc, prm, nthreads=4)
    _, rlin, _ = oracle.render(sc, prm, nthreads=4, linear=True)
    return r8, rlin, shadow


def same_bits_or_both_nan(a, b):
    """Bit for bit, a NaN on both sides counting as equal (the host's default NaN carries the sign bit,
    the device's does not)."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check_frame(rt, objs, lights, cam, ref, jit_active, what):
    r8, rlin, rshadow = ref
    g8, glin = rt.render_f32(objs, lights, [], cam, linear=True)
    st = rt.stats()
    ok = same_bits_or_both_nan(glin, rlin)
    assert ok.all(), (what, "linear image", np.flatnonzero(~ok)[:8] // 4, glin.reshape(-1)[~ok][:8], rlin.reshape(-1)[~ok][:8])
    assert int(st.shadow_rays) == rshadow, (what, "shadow rays", int(st.shadow_rays), rshadow)
    d8 = np.abs(g8.astype(np.int16).reshape(-1) - r8.astype(np.int16).reshape(-1))
    assert d8.max() <= 1, (what, "rgba8", np.flatnonzero(d8 > 1)[:8] // 4)
    assert st.jit_active == jit_active, (what, "kernel path", st.jit_active)


# variant -> (JIT policy, RRTE_JIT_TOPO, the jit_active the frame must report: 1 full, 2 topology kernel)
VARIANTS = {"generic": (abi.JIT_OFF, None, 0), "jit-full": (abi.JIT_ON, "0", 1), "jit-topology": (abi.JIT_ON, "1", 2)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_edge_frames_match_the_oracle(scene, mode, variant, monkeypatch, tmp_path):
    jit, topo, active = VARIANTS[variant]
    if topo is not None:
        monkeypatch.setenv("RRTE_JIT_TOPO", topo)
        monkeypatch.setenv("RRTE_JIT_CACHE_DIR", str(tmp_path))  # one compile for the four contexts below
    objs, lights = SCENES[scene]()
    shadow_total = nan_pixels = 0
    for cull, tile in itertools.product("01", "01"):
        monkeypatch.setenv("RRTE_CULL", cull)
        monkeypatch.setenv("RRTE_TILE_CULL", tile)
        for w, h in SIZES:
            rt = Raytracer(config(w, h, mode), device=0, jit=jit)
            for name, cam in cameras(w, h).items():
                ref = want(scene, mode, name, w, h)
                shadow_total += ref[2]
                nan_pixels += int(np.isnan(ref[1]).any(-1).sum())
                check_frame(rt, objs, lights, cam, ref, active,
                            f"{scene} {mode} {variant} cull={cull} tile={tile} {w}x{h} {name}")
            rt.ctx.close()
    print(f"{scene} {mode} {variant}: oracle shadow rays {shadow_total}, pixels with a NaN channel {nan_pixels}")
    if mode == "lambert_shadow":
        assert shadow_total > 0


def test_edge_frames_are_not_vacuous():
    """From the oracle alone: the -z orthographic frame of the analytic grid sees every object, the
    cameras see different frames, and the shadowed mode casts shadow rays."""
    objs, lights = analytic_grid()
    cam = cameras(16, 16)["ortho-z"]
    sc = LoweredScene(objs, lights, cam)
    import query_ref as q
    ys, xs = np.divmod(np.arange(256), 16)
    rays = q.oracle_pick_rays(sc, 16, 16, xs, ys, 1e-3)
    assert (rays["direction"] == np.array([0, 0, -1], np.float32)).all()
    assert (np.modf(rays["origin"] * 8)[0] == 0).all()
    hit = q.oracle_closest(sc, rays)
    assert set(hit["prim"]) == set(range(7))
    on_sphere = hit["prim"] == 0
    assert hit["t"][on_sphere].min() == np.float32(8 - 0.625)  # pixel (3, 3) hits the point the light sits on
    lins = [want("analytic", "lambert_shadow", c, 16, 16)[1].tobytes() for c in CAMERAS]
    assert len(set(lins)) >= len(CAMERAS) - 2  # (from behind, the plane fills two of the frames alike)
    assert want("analytic", "lambert_shadow", "ortho-z", 16, 16)[2] > 100


@functools.lru_cache(maxsize=None)
def _instance_frames(mode):
    """The instance scene's two perspective frames and their reference: numpy_ref.render with the
    instance checker (instance_ref.render patches numpy_ref for the length of the call)."""
    objs, lights = sdf_grid(instance=True)
    w, h = 24, 16
    out = []
    for name in ("eye-in-cube", "eye-at-sphere-centre"):
        cam = cameras(w, h)[name]
        cam.transform.position = vec3(cam.transform.position[0], cam.transform.position[1], 6.0)  # step back: the grid in view
        cfg = config(w, h, mode)
        with pytest.MonkeyPatch.context() as mp:
            r8, _, rshadow = instance_ref.render(mp, LoweredScene(objs, lights, cam), cfg.lower(), linear=False)
            _, rlin, _ = instance_ref.render(mp, LoweredScene(objs, lights, cam), cfg.lower(), linear=True)
        out.append((name, cam, cfg, (r8.reshape(-1), rlin, rshadow)))
    return objs, lights, out


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
def test_instance_in_the_sdf_grid(mode, variant, monkeypatch, tmp_path):
    """The SDF grid with a mirrored, non-uniformly scaled instance of its mesh, point lights only,
    through the perspective cameras, in both modes, with every kernel variant and RRTE_CULL and
    RRTE_TILE_CULL off and on: against the numpy restatement with the instance checker (the C oracle
    has no instance kind, the restatement no orthographic camera and no directional light)."""
    jit, topo, active = VARIANTS[variant]
    if topo is not None:
        monkeypatch.setenv("RRTE_JIT_TOPO", topo)
        monkeypatch.setenv("RRTE_JIT_CACHE_DIR", str(tmp_path))
    objs, lights, frames = _instance_frames(mode)
    if mode == "lambert_shadow":
        assert all(ref[2] > 0 for _, _, _, ref in frames)
    for cull, tile in itertools.product("01", "01"):
        monkeypatch.setenv("RRTE_CULL", cull)
        monkeypatch.setenv("RRTE_TILE_CULL", tile)
        for name, cam, cfg, ref in frames:
            rt = Raytracer(cfg, device=0, jit=jit)
            check_frame(rt, objs, lights, cam, ref, active, f"instance {mode} {variant} cull={cull} tile={tile} {name}")
            rt.ctx.close()


def huge_plane_scene(w, h):
    """A plane at y = -2^65 under a unit sphere at the origin, lit from straight above.  Every shadow
    ray from the plane starts about 2^65 from the sphere and moves towards it: hb*hb and a*cc both
    overflow, the reference's discriminant is NaN, all its comparisons fail and it reports the ray
    occluded -- also for points far to the side, whose rays pass nowhere near the sphere."""
    objs = [Sphere((0.0, 0.0, 0.0), 1.0, eb.MAT), Plane((0.0, -float(2.0 ** 65), 0.0), (0.0, 1.0, 0.0), eb.MAT2)]
    lights = [DirectionalLight((0.0, -1.0, 0.0), WHITE, 1.0)]
    cam = Camera.new_perspective(to_radians(60.0), w / h, 0.1, 100.0)
    cam.transform.position = vec3(0.0, 1.0, 5.0)
    cam.look_at((0.0, -1.0, 0.0))
    return objs, lights, cam


def far_sphere_below_scene(w, h):
    """The same light over an ordinary plane y = 0, and a unit sphere 2^66 below it: every shadow ray
    leaves the plane upwards, away from the sphere (hb = 2^66 > 0, cc = +inf > 0) -- the any-hit
    early-out's case -- and the reference, whose hb*hb and a*cc are both +inf, reports it occluded."""
    objs = [Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), eb.MAT2), Sphere((0.0, -float(2.0 ** 66), 0.0), 1.0, eb.MAT)]
    lights = [DirectionalLight((0.0, -1.0, 0.0), WHITE, 1.0)]
    cam = Camera.new_perspective(to_radians(60.0), w / h, 0.1, 100.0)
    cam.transform.position = vec3(0.0, 2.0, 5.0)
    cam.look_at((0.0, 0.0, 0.0))
    return objs, lights, cam


EXTREME = {"plane-2^65-below-the-sphere": (huge_plane_scene, 1), "sphere-2^66-below-the-plane": (far_sphere_below_scene, 0)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("scene", list(EXTREME))
def test_shadow_frame_at_extreme_scale(scene, variant, monkeypatch, tmp_path):
    """The confirmed leaves_sphere / culling case in the shadow path: with RRTE_CULL on and off the
    frame is the oracle's, whose plane pixels are all in the sphere's "shadow".

    Against the library of the commit before the early-out was bounded, the second scene fails (its
    plane comes out lit: leaves_sphere answers "miss") and the first passes: there the shadow rays
    move towards the sphere, so the early-out does not apply, and the cull's own hit bound overflows
    to an infinite radius, which keeps every object."""
    jit, topo, active = VARIANTS[variant]
    if topo is not None:
        monkeypatch.setenv("RRTE_JIT_TOPO", topo)
        monkeypatch.setenv("RRTE_JIT_CACHE_DIR", str(tmp_path))
    w, h = 16, 16
    build, plane = EXTREME[scene]
    objs, lights, cam = build(w, h)
    cfg = config(w, h, "lambert_shadow")
    sc = LoweredScene(objs, lights, cam)
    r8, _, rshadow = oracle.render(sc, cfg.lower(), nthreads=4)
    _, rlin, _ = oracle.render(sc, cfg.lower(), nthreads=4, linear=True)
    import query_ref as q
    ys, xs = np.divmod(np.arange(w * h), w)
    first = q.oracle_closest(sc, q.oracle_pick_rays(sc, w, h, xs, ys, cfg.t_min))
    on_plane = first["prim"] == plane
    assert on_plane.sum() >= 50 and rshadow >= on_plane.sum()
    # every plane pixel is shadowed: its colour is the ambient term alone, one value for all of them
    assert len(set(map(bytes, rlin.reshape(-1, 4)[on_plane]))) == 1
    for cull in "01":
        monkeypatch.setenv("RRTE_CULL", cull)
        rt = Raytracer(cfg, device=0, jit=jit)
        check_frame(rt, objs, lights, cam, (r8, rlin, rshadow), active, f"{scene} {variant} cull={cull}")
        rt.ctx.close()
