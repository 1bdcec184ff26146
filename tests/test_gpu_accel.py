"""The scene accelerator on the device (include/rrte_hip_accel.h): a top-level tree over
the objects that only culls, so everything an accelerated context renders or answers must be bit for
bit what the linear scan gives -- checked against the oracle's linear scan (oracle.render,
query_ref; instance_ref for scenes with mesh instances).  The unaccelerated device is the reference
only where the oracle cannot be one bit for bit (REFCOMPAT beyond depth 2, test_bounce_rays_walk) and
where a test is about the device agreeing with itself (peers, bands, policy switches).

Contexts use set_scene_accel(ON, min_prims=1) unless a test says otherwise, so that small scenes --
whose reference frames stay quick -- run the accelerated kernels too."""
import ctypes as C
import math

import numpy as np
import pytest

import edge_bank as eb
import instance_ref as ir
import oracle
import query_ref as q
from rrte_amd import (Camera, Capsule, Color, CSGComposite, Cube, DeformedSDF, LambertianMaterial, LoweredScene,
                      MeshInstance, Plane, PointLight, Raytracer, RaytracerConfig, SDFBox, SDFObject, SDFSphere,
                      Sphere, Transform, abi, scenes)
from rrte_amd.mesh import icosphere
from rrte_amd.renderer import Context, TwistDeformer
from test_accel_cpu import build_tool, dump

pytestmark = pytest.mark.gpu

F = np.float32
ON, OFF = abi.SCENE_ACCEL_ON, abi.SCENE_ACCEL_OFF


def _mat(r, g, b):
    return LambertianMaterial(Color.rgb(r, g, b))


def _lights():
    return [PointLight((-10.0, 15.0, 10.0), Color.rgb(1.0, 1.0, 1.0), 25.0),
            PointLight((10.0, 10.0, 15.0), Color.rgb(0.6, 0.7, 1.0), 15.0)]


def accel_ctx(min_prims=1, flags=0, jit=abi.JIT_OFF):
    ctx = Context(0, jit=jit)
    ctx.set_scene_accel(ON, min_prims, flags)
    return ctx


def cfg_of(w, h, mode="lambert_shadow", **kw):
    kw = {"max_depth": 1, "samples_per_pixel": 1, "jitter": "center", **kw}
    return RaytracerConfig(width=w, height=h, mode=mode, **kw)


def cam_of(w, h):
    return scenes._camera(w, h, (0.0, 9.0, 13.0), (0.0, 0.5, -5.0))


def _slot(i):
    return ((i % 10) - 4.5) * 1.7, 2.0 - (i // 10) * 1.7


def mix(n, instances):
    """n objects on a grid, the kind chosen by index modulo: spheres, cubes, capsules, one-leaf and CSG
    SDF objects, a deformer object, plain meshes and (with `instances`) instances of one base mesh.  A
    plane at index 0 and, from three objects on, another at the last index; one object is one sphere."""
    base = icosphere((0.0, 0.0, 0.0), 0.6, 1, _mat(0.8, 0.3, 0.3))
    objs = []
    for i in range(n):
        x, z = _slot(i)
        m = _mat(0.25 + 0.07 * (i % 10), 0.3 + 0.05 * (i % 13), 0.9 - 0.06 * (i % 11))
        if (i == 0 and n >= 2) or (i == n - 1 and n >= 3):
            objs.append(Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), m) if i == 0 else Plane((0.0, 0.0, -26.0), (0.0, 0.0, 1.0), m))
            continue
        k = i % 9
        if k in (0, 8):
            objs.append(Sphere((x, 0.6, z), 0.6, m))
        elif k == 1:
            cube = Cube((x, 0.6, z), (1.0, 1.2, 0.8), m)
            cube.set_transform(Transform((0.0, 0.0, 0.0), scenes.Q_Y45, (1.0, 1.0, 1.0)))
            objs.append(cube)
        elif k == 2:
            objs.append(Capsule((x, 0.8, z), 0.35, 1.0, m))
        elif k == 3:
            objs.append(SDFObject(SDFSphere((x, 0.6, z), 0.6), m))
        elif k == 4:
            objs.append(SDFObject(CSGComposite.smooth_union(SDFSphere((x - 0.2, 0.5, z), 0.45), SDFBox((x + 0.25, 0.5, z), (0.6, 0.8, 0.6)), 0.2), m))
        elif k == 5:
            objs.append(SDFObject(DeformedSDF(SDFBox((x, 0.7, z), (0.6, 1.2, 0.6)), TwistDeformer((0.0, 1.0, 0.0), 1.5, (x, 0.7, z))), m))
        elif k == 6 or not instances:
            objs.append(icosphere((x, 0.6, z), 0.6, 0 if i % 2 else 1, m))
        else:
            objs.append(MeshInstance(base, Transform((x, 0.6, z), scenes.Q_X45 if i % 2 else scenes.Q_Y45, (1.0, 0.7, 1.2)), m))
    return objs


def _render(ctx, sc, prm, linear=True):
    p = abi.RenderParams.from_buffer_copy(prm)
    if linear:
        p.flags |= abi.FLAG_F32_LINEAR
    n = p.width * p.height * 4
    out8, outf = np.empty(n, np.uint8), np.empty(n, np.float32)
    ctx.check(ctx.lib.rrte_hip_render_f32(ctx.h, sc.ref(), C.byref(p), out8.ctypes.data, outf.ctypes.data))
    return out8, outf, ctx.stats()


_want = {}


def _oracle_frame(key, sc, prm, render=None):
    """The reference frame of a scene, computed once per key: (rgba8, linear f32, shadow rays).
    `render`: instance_ref's checker for scenes with instances (the C oracle has plain meshes only)."""
    if key not in _want:
        if render is None:
            r8, _, _ = oracle.render(sc, prm, nthreads=8)
            _, lin, shadow = oracle.render(sc, prm, nthreads=8, linear=True)
        else:
            r8, _, _ = render(sc, prm, False)
            _, lin, shadow = render(sc, prm, True)
        r8, lin = r8.reshape(-1), lin.reshape(-1)
        for a in (r8, lin):
            a.setflags(write=False)
        _want[key] = (r8, lin, shadow)
    return _want[key]


def _check_frame(ctx, sc, prm, want, lambert=True):
    """The existing compare rule: linear image and shadow-ray count identical, RGBA8 within 1."""
    r8, lin, shadow = want
    _, glin, st = _render(ctx, sc, prm)
    assert st.jit_active == 0
    bad = np.flatnonzero(glin.view(np.uint32) != lin.view(np.uint32))
    assert bad.size == 0, (bad.size, bad[:8] // 4, glin[bad[:8]], lin[bad[:8]])
    if lambert:
        assert int(st.shadow_rays) == shadow
    g8, _, _ = _render(ctx, sc, prm, linear=False)
    assert np.abs(g8.astype(np.int16) - r8.astype(np.int16)).max() <= 1
    return g8


def _raycast(ctx, sc, rays, any_hit, pad=0):
    hits = np.zeros(len(rays) + pad, dtype=abi.RAY_HIT_DTYPE)
    hits.view(np.uint8)[:] = 0xA5
    ctx.check(ctx.lib.rrte_hip_raycast(ctx.h, sc.ref(), rays.ctypes.data_as(C.POINTER(abi.Ray)), len(rays),
                                       abi.QUERY_ANY if any_hit else abi.QUERY_CLOSEST,
                                       hits.ctypes.data_as(C.POINTER(abi.RayHit))))
    assert (hits.view(np.uint8)[len(rays) * hits.itemsize:] == 0xA5).all(), "records behind the hits were written"
    return hits[:len(rays)]


# ------------------------------------------------------------------- 1. engages and reports
def _tiny_far_spheres(n):
    """n degenerate spheres far behind the camera of cam_of, plus nothing else."""
    return [Sphere((float(i % 128) * 0.01, 50.0 + (i // 128) * 0.01, 60.0), 1e-4, _mat(0.5, 0.5, 0.5)) for i in range(n)]


def test_engages_and_reports():
    ctx = Context(0, jit=abi.JIT_OFF)
    a = ctx.accel_info()
    assert (a.policy, a.min_prims, a.flags) == (OFF, 65, 0)
    assert (a.builds, a.fallbacks, a.nodes, a.depth, a.bounded, a.unbounded, a.searches, a.candidates) == (0,) * 8
    for bad in [(2, 0, 0), (ON, 0, 2), (ON, 0, 0x80000001), (0xFFFFFFFF, 0, 0)]:
        assert ctx.lib.rrte_hip_set_scene_accel(ctx.h, *bad) == abi.RRTE_INVALID_ARG, bad
    a = ctx.accel_info()
    assert (a.policy, a.min_prims, a.flags) == (OFF, 65, 0)
    ctx.set_scene_accel(ON)  # default min_prims
    assert ctx.accel_info().min_prims == 65
    w, h = 64, 36
    prm = cfg_of(w, h).lower()
    sc64, sc65 = (LoweredScene(mix(n, False), _lights(), cam_of(w, h)) for n in (64, 65))
    _check_frame(ctx, sc64, prm, _oracle_frame(("mix", 64, w, h, "lambert_shadow"), sc64, prm))
    a = ctx.accel_info()
    assert (a.nodes, a.depth, a.bounded, a.unbounded, a.builds, a.fallbacks) == (0, 0, 0, 0, 0, 0)
    _check_frame(ctx, sc65, prm, _oracle_frame(("mix", 65, w, h, "lambert_shadow"), sc65, prm))
    a = ctx.accel_info()
    assert a.nodes > 0 and 1 <= a.depth <= 32 and (a.bounded, a.unbounded) == (63, 2) and (a.builds, a.fallbacks) == (1, 0)
    assert (a.searches, a.candidates) == (0, 0)  # counting is off
    # all planes: nothing has a finite bound -- a fallback that renders the oracle's frame
    ctx.set_scene_accel(ON, 1)
    planes = [Plane((0.0, -1.0 - i, 0.0), (0.0, 1.0, 0.0), _mat(0.5, 0.2 * i, 0.5)) for i in range(3)]
    scp = LoweredScene(planes, _lights(), cam_of(w, h))
    _check_frame(ctx, scp, prm, _oracle_frame(("planes", w, h), scp, prm))
    a = ctx.accel_info()
    assert (a.nodes, a.bounded, a.unbounded, a.builds, a.fallbacks) == (0, 0, 0, 1, 1)
    # one object too many: a fallback; one fewer is accelerated (degenerate spheres off screen, 16x9)
    prm9 = cfg_of(16, 9).lower()
    ground = [Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.5, 0.5, 0.5)), Sphere((0.0, 1.0, -4.0), 1.0, _mat(0.9, 0.2, 0.2))]
    big = LoweredScene(ground + _tiny_far_spheres(abi.ACCEL_MAX_PRIMS + 1 - 2), _lights(), cam_of(16, 9))
    assert big.ir.num_prims == 16385
    _check_frame(ctx, big, prm9, _oracle_frame(("big", 16385), big, prm9))
    a = ctx.accel_info()
    assert (a.nodes, a.builds, a.fallbacks) == (0, 1, 2)
    full = LoweredScene(ground + _tiny_far_spheres(abi.ACCEL_MAX_PRIMS - 2), _lights(), cam_of(16, 9))
    _check_frame(ctx, full, prm9, _oracle_frame(("big", 16384), full, prm9))
    a = ctx.accel_info()
    assert a.nodes > 0 and a.bounded == 16384 and (a.builds, a.fallbacks) == (2, 2)
    ctx.close()


def test_the_environment_form_and_the_jit_policy(monkeypatch):
    monkeypatch.setenv("RRTE_SCENE_ACCEL", "on")
    monkeypatch.setenv("RRTE_SCENE_ACCEL_MIN", "3")
    ctx = Context(0, jit=abi.JIT_ON)
    a = ctx.accel_info()
    assert (a.policy, a.min_prims) == (ON, 3)
    w, h = 64, 36
    prm = cfg_of(w, h).lower()
    sc = LoweredScene(mix(5, False), _lights(), cam_of(w, h))
    # JIT ON would specialise this scene; accelerated, it runs the generic variant
    _check_frame(ctx, sc, prm, _oracle_frame(("mix", 5, w, h, "lambert_shadow"), sc, prm))
    assert ctx.accel_info().bounded == 3
    ctx.set_scene_accel(OFF)
    _, _, st = _render(ctx, sc, prm)
    assert st.jit_active != 0 and ctx.accel_info().nodes == 0
    ctx.close()


# ----------------------------------------------------------------- 2. frames equal the oracle
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 130]


@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
@pytest.mark.parametrize("n", SIZES)
def test_frames_equal_the_oracle(n, mode):
    ctx = accel_ctx()
    for w, h in [(64, 36), (67, 37)]:
        sc, prm = LoweredScene(mix(n, False), _lights(), cam_of(w, h)), cfg_of(w, h, mode).lower()
        _check_frame(ctx, sc, prm, _oracle_frame(("mix", n, w, h, mode), sc, prm), mode == "lambert_shadow")
        a = ctx.accel_info()
        planes = 0 if n == 1 else 1 if n == 2 else 2
        assert (a.bounded, a.unbounded, a.fallbacks) == (n - planes, planes, 0)
    ctx.close()


def _instance_frame(key, sc, prm, monkeypatch):
    """_oracle_frame through instance_ref's numpy checker, rendered ONCE: the checker's linear frame, and
    its RGBA8 frame formed from that with numpy_ref.render's own closing lines (gamma, clamp, quantise)."""
    if key not in _want:
        _, lin, shadow = ir.render(monkeypatch, sc, prm, True)
        inv_g = F(1) / F(prm.gamma)
        with np.errstate(invalid="ignore"):
            g = [np.power(lin[..., k], inv_g) if k < 3 else lin[..., k] for k in range(4)]
            g = [np.where(np.isnan(x), x, np.clip(x, F(0), F(1))) for x in g]
            qs = [np.where(~(x * F(255) > F(0)), 0, np.where(x * F(255) >= F(255), 255, np.nan_to_num(x * F(255)).astype(np.int64)))
                  for x in g]
        r8, lin = np.stack(qs, -1).astype(np.uint8).reshape(-1), lin.reshape(-1)
        for a in (r8, lin):
            a.setflags(write=False)
        _want[key] = (r8, lin, shadow)
    return _want[key]


# The mix WITH mesh instances, which the C oracle does not have, so the checker is instance_ref's numpy
# one.  It costs seconds per frame at 64x36 and grows with objects x pixels, so the larger scenes use
# smaller frames -- still ragged (no multiple of the 8x8 tile) and several tiles -- not fewer cases.
INSTANCE_FRAMES = [(33, 67, 37), (65, 35, 19), (130, 19, 11)]


@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
@pytest.mark.parametrize("n,w,h", INSTANCE_FRAMES)
def test_frames_with_instances_equal_the_checker(n, w, h, mode, monkeypatch):
    sc, prm = LoweredScene(mix(n, True), _lights(), cam_of(w, h)), cfg_of(w, h, mode).lower()
    inst = [i for i in range(n) if sc.prims[i].kind == abi.PRIM_MESH_INSTANCE]
    assert len(inst) >= 3 and (n < 65 or max(inst) >= 32) and (n < 130 or max(inst) >= 96)
    want = _instance_frame(("mixi", n, w, h, mode), sc, prm, monkeypatch)
    ctx = accel_ctx()
    _check_frame(ctx, sc, prm, want, mode == "lambert_shadow")
    assert ctx.accel_info().nodes > 0
    ctx.close()


@pytest.mark.parametrize("n", [33, 65])
def test_bounce_rays_walk(n):
    """REFCOMPAT with spp 2, random jitter and scatter, so that every bounce ray walks the tree.

    Depth 2 is compared with the oracle bit for bit.  Depth 3 cannot be: the device evaluates the
    reference's recursion forward, which is exact up to depth 2 and differs at rounding level beyond
    (shade.hpp PathState; tests/test_gpu_parity.py test_stochastic_multibounce_materials), with
    or without the accelerator -- measured on the 33-object scene, 901 of 9216 floats differ from the
    oracle by one ulp under policy OFF and the same 901 under ON.  So at depth 3 the frame must be
    bit for bit the same context's frame under policy OFF, and meet the oracle under the rule the
    existing multi-bounce tests use (rms <= RMS_TOL on the f32 frame, RGBA8 within 1)."""
    from test_gpu_parity import RMS_TOL
    w, h = 64, 36
    waves = math.ceil(w / 8) * math.ceil(h / 8)
    sc = LoweredScene(mix(n, False), _lights(), cam_of(w, h))
    ctx = accel_ctx(flags=abi.ACCEL_COUNT)
    prm2 = cfg_of(w, h, "refcompat", max_depth=2, samples_per_pixel=2, jitter="random").lower()
    _check_frame(ctx, sc, prm2, _oracle_frame(("bounce2", n), sc, prm2), False)
    a = ctx.accel_info()
    assert a.searches > 2 * waves, "no bounce ray walked"
    prm3 = cfg_of(w, h, "refcompat", max_depth=3, samples_per_pixel=2, jitter="random").lower()
    _, on_lin, _ = _render(ctx, sc, prm3)
    on8, on_f, _ = _render(ctx, sc, prm3, linear=False)
    assert ctx.accel_info().searches > a.searches / 2 and ctx.accel_info().nodes > 0
    ctx.set_scene_accel(OFF)
    _, off_lin, _ = _render(ctx, sc, prm3)
    assert ctx.accel_info().nodes == 0
    r8, rf, _ = oracle.render(sc, prm3, nthreads=8)
    _, rlin, _ = oracle.render(sc, prm3, nthreads=8, linear=True)
    print(f"depth 3, {n} objects: floats differing from the oracle: OFF "
          f"{int((off_lin.view(np.uint32) != rlin.reshape(-1).view(np.uint32)).sum())}, ON "
          f"{int((on_lin.view(np.uint32) != rlin.reshape(-1).view(np.uint32)).sum())}")
    assert np.array_equal(on_lin.view(np.uint32), off_lin.view(np.uint32))
    d = on_f.astype(np.float64) - rf.reshape(-1).astype(np.float64)
    assert float(np.sqrt(np.mean(d ** 2))) <= RMS_TOL
    assert np.abs(on8.astype(np.int16) - r8.reshape(-1).astype(np.int16)).max() <= 1
    ctx.close()


# ---------------------------------------------------------------- 3. ties across the mask
def tie_scene():
    """72 objects: small distinct filler spheres, and at indices 3 / 40 identical spheres, at 5 an analytic
    sphere whose SDF twin is at 70, at 31 / 32 coplanar duplicate instances (the mask's first dword edge)."""
    base = icosphere((0.0, 0.0, 0.0), 0.8, 1, _mat(0.2, 0.8, 0.3))
    objs = []
    for i in range(72):
        x, z = _slot(i)
        objs.append(Sphere((x, 0.3, z - 8.0), 0.3, _mat(0.3 + 0.005 * i, 0.4, 0.6)))
    objs[3] = Sphere((-3.0, 1.0, 0.0), 1.0, _mat(0.9, 0.1, 0.1))
    objs[40] = Sphere((-3.0, 1.0, 0.0), 1.0, _mat(0.1, 0.9, 0.1))
    objs[5] = Sphere((0.0, 1.0, 0.0), 1.0, _mat(0.9, 0.9, 0.1))
    objs[70] = SDFObject(SDFSphere((0.0, 1.0, 0.0), 1.0), _mat(0.1, 0.1, 0.9))
    tr = Transform((3.0, 1.0, 0.0), scenes.Q_Y45, (1.0, 1.2, 1.0))
    objs[31] = MeshInstance(base, tr, _mat(0.8, 0.2, 0.8))
    objs[32] = MeshInstance(base, tr, _mat(0.2, 0.8, 0.8))
    return objs


def test_ties_across_the_mask(monkeypatch):
    objs = tie_scene()
    sc = LoweredScene(objs, [], Camera())
    rng = np.random.default_rng(11)
    tg = np.concatenate([c + rng.uniform(-0.9, 0.9, (60, 3)) for c in ([-3.0, 1.0, 0.0], [0.0, 1.0, 0.0], [3.0, 1.0, 0.0])])
    o = (tg + rng.uniform(-1.0, 1.0, tg.shape) + [0.0, 3.0, 9.0]).astype(F)
    d = (tg - o).astype(F)
    rays = q.rays_of(o, d)
    want = ir.closest(sc, rays)
    won = {int(p) for p in want["prim"]}
    # the lower index wins the exact ties; the SDF twin reports its march's t (just short of the analytic
    # root), so the pair 5 / 70 is a near-tie that the narrowed t_max of the SDF object decides
    assert {3, 31} <= won and (won & {5, 70}) and not ({40, 32} & won), won
    ctx = accel_ctx()
    q.assert_hits_equal(_raycast(ctx, sc, rays, False), want, tri=True)
    assert ctx.accel_info().nodes > 0
    w, h = 64, 36
    scf, prm = LoweredScene(objs, _lights(), scenes._camera(w, h, (0.0, 3.0, 10.0), (0.0, 1.0, 0.0))), cfg_of(w, h).lower()
    _check_frame(ctx, scf, prm, _oracle_frame(("ties", w, h), scf, prm, lambda s, p, lin: ir.render(monkeypatch, s, p, lin)))
    ctx.close()


# ----------------------------------------------------------------------------- 4. queries
@pytest.fixture(scope="module")
def query_case():
    sc = LoweredScene(mix(65, True), [], Camera())
    o, d, length = q.gen_rays()
    t_max = np.where(np.arange(len(o)) % 3 == 0, length * F(0.8), q.INF).astype(F)
    # the generator's box is [-12, 12] x [0.2, 9] x [-12, 12]: moved over the grid of objects
    o = (o + np.array([0.0, 0.0, -4.0], F)).astype(F)
    rays = q.rays_of(o, d, q.T_MIN, t_max)
    seg = rays.copy()
    seg["t_max"] = np.where(np.isinf(t_max), length * F(1.5), t_max)  # ANY: finite segments only
    return sc, rays, ir.closest(sc, rays), seg, ir.any_hit(sc, seg)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 517])
def test_queries(query_case, n):
    sc, rays, want_c, seg, want_a = query_case
    assert (want_c["prim"] >= 0).sum() > 100 and len({int(p) for p in want_c["prim"]}) > 15
    assert (want_a["prim"] >= 0).sum() > 60 and np.isfinite(seg["t_max"]).all()
    ctx = accel_ctx()
    q.assert_hits_equal(_raycast(ctx, sc, rays[:n].copy(), False, pad=64), want_c[:n], tri=True)
    q.assert_hits_equal(_raycast(ctx, sc, seg[:n].copy(), True, pad=64), want_a[:n], tri=True)
    assert ctx.accel_info().nodes > 0
    ctx.close()


def test_pick():
    w, h = 33, 19
    objs = mix(65, True)
    cam = cam_of(w, h)
    ys, xs = (a.ravel() for a in np.mgrid[0:h, 0:w])
    rt = Raytracer(RaytracerConfig(width=w, height=h), device=0, jit=abi.JIT_OFF, scene_accel=ON, accel_min_prims=1)
    got = rt.pick(objs, cam, xs, ys)
    sc = LoweredScene(objs, [], cam)
    want = ir.closest(sc, q.oracle_pick_rays(sc, w, h, xs, ys, rt.config.t_min))
    assert len({int(p) for p in want["prim"]}) >= 10 and rt.ctx.accel_info().nodes > 0
    q.assert_hits_equal(got, want, tri=True)
    rt.ctx.close()


# ------------------------------------------------------------- 5. the edge-case ray bank
@pytest.fixture(scope="module")
def accel_rt():
    r = Raytracer(device=0, scene_accel=ON, accel_min_prims=1)
    yield r
    r.ctx.close()


@pytest.mark.parametrize("tier,group", eb.CASES, ids=[f"{t}-{g}" for t, g in eb.CASES])
def test_edge_bank_with_the_accelerator(accel_rt, tier, group):
    """Single-object scenes give a root-leaf tree (planes and rejected data none: a fallback);
    non-finite and far rays exercise the stand-downs.  Same rules as tests/test_gpu_edge_bank.py."""
    from test_gpu_edge_bank import check
    _, _, rays, _, sc = eb.case(tier, group)
    wc, wa = eb.want_closest(tier, group), eb.want_any(tier, group)
    assert int(eb.non_finite(wc).sum()) == eb.NON_FINITE[(tier, group)]
    ctx = accel_rt.ctx
    check(tier, group, _raycast(ctx, sc, rays, False), wc, tri=eb.has_instance(sc))
    check(tier, group, _raycast(ctx, sc, rays, True), wa, tri=True)
    a = ctx.accel_info()
    assert a.policy == ON and a.bounded + a.unbounded in (0, sc.ir.num_prims)


# ----------------------------------------------------------------- 6. change and lifetime
def family(w, h):
    ball = icosphere((0.0, 1.0, 0.0), 1.0, 1, _mat(0.8, 0.3, 0.3))
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.5, 0.5, 0.5)), ball,
            MeshInstance(ball, Transform((-3.0, 0.0, 0.5), scenes.Q_Y90, (1.0, 1.0, 1.0))),
            MeshInstance(ball, Transform((3.0, 0.2, 0.0), scenes.Q_X45, (0.7, 1.4, 0.7)), _mat(0.3, 0.7, 0.4)),
            Sphere((-1.5, 0.6, 3.5), 0.6, _mat(0.9, 0.8, 0.2)), Cube((1.5, 0.5, 3.0), (1.0, 1.0, 1.0), _mat(0.2, 0.3, 0.9))]
    return ball, objs, scenes._camera(w, h, (0.0, 5.0, 11.0), (0.0, 1.0, 0.0))


def test_moving_an_instance_rebuilds_the_top_level_only(monkeypatch):
    w, h = 64, 36
    _, objs, cam = family(w, h)
    sc, prm = LoweredScene(objs, _lights(), cam), cfg_of(w, h).lower()
    ctx = accel_ctx()
    for k in range(3):
        sc.prims[3].trs[0] = 3.0 - 1.1 * k
        sc.prims[3].trs[2] = 0.7 * k
        want = _oracle_frame(("move", k), sc, prm, lambda s, p, lin: ir.render(monkeypatch, s, p, lin))
        _check_frame(ctx, sc, prm, want)
        assert (ctx.accel_info().builds, ctx.mesh_info().bvh_builds) == (k + 1, 1)
    ctx.close()


def test_four_frames_in_flight_each_see_their_own_tree():
    import torch
    w, h = 64, 36
    prm = cfg_of(w, h).lower()
    scs, plain = [], []
    for k in range(4):
        objs = mix(33, False)
        objs[12] = Sphere((-6.0 + 4.0 * k, 1.5, 1.0 - 2.0 * k), 1.5, _mat(0.9, 0.1, 0.1))
        sc = LoweredScene(objs, _lights(), cam_of(w, h))
        scs.append(sc)
        plain.append(_oracle_frame(("flight", k), sc, prm)[0])
    assert all(not np.array_equal(plain[0], p) for p in plain[1:])
    ctx = accel_ctx()
    bufs = [torch.zeros(w * h, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for sc, buf in zip(scs, bufs):
        ctx.check(ctx.lib.rrte_hip_render_async(ctx.h, sc.ref(), C.byref(prm), buf.data_ptr(), None, None))
    ctx.check(ctx.lib.rrte_hip_synchronize(ctx.h))
    assert ctx.accel_info().builds == 4
    for k, buf in enumerate(bufs):
        got = buf.cpu().numpy().view(np.uint8)
        assert np.abs(got.astype(np.int16) - plain[k].astype(np.int16)).max() <= 1, k
    ctx.close()


def test_a_refit_of_an_instanced_mesh(monkeypatch):
    w, h = 64, 36
    ball, objs, cam = family(w, h)
    rt = Raytracer(cfg_of(w, h), device=0, jit=abi.JIT_OFF, scene_accel=ON, accel_min_prims=1)
    rt.render(objs, _lights(), [], cam)
    p = ball.positions.astype(np.float64)
    ball.set_vertices((p * np.array([1.3, 0.8, 1.1]) + np.stack([0.2 * np.sin(3.0 * p[:, 1]), 0.0 * p[:, 0], 0.1 * p[:, 0]], 1)).astype(F))
    _, glin = rt.render_f32_deformed(objs, _lights(), [], cam, linear=True)
    assert rt.ctx.refit_info().device_refits == 1 and rt.ctx.accel_info().builds == 2
    sc, prm = LoweredScene(objs, _lights(), cam), cfg_of(w, h).lower()
    want = _oracle_frame(("refit",), sc, prm, lambda s, p_, lin: ir.render(monkeypatch, s, p_, lin))
    assert np.array_equal(np.asarray(glin).reshape(-1).view(np.uint32), want[1].view(np.uint32))
    rt.ctx.close()


@pytest.mark.parametrize("nranks,band", [(2, 8), (4, 16), (8, 16)])
def test_emulated_peers_and_bands_are_the_plain_render(nranks, band, monkeypatch):
    import torch
    w, h = 320, 180
    sc, prm = LoweredScene(mix(65, True), _lights(), cam_of(w, h)), cfg_of(w, h).lower()
    prm.band_rows = band
    ctx = accel_ctx()
    plain = np.zeros(w * h * 4, dtype=np.uint8)
    ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), plain.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert ctx.accel_info().nodes > 0
    ctx.close()
    assert len(np.unique(plain.reshape(-1, 4), axis=0)) > 100
    monkeypatch.setenv("RRTE_FORCE_GATHER", "1")
    monkeypatch.setenv("RRTE_EMULATE_PEERS", str(nranks))
    ctx = accel_ctx()
    lib = ctx.lib
    uid = (C.c_uint8 * abi.UNIQUE_ID_BYTES)()
    ctx.check(lib.rrte_hip_comm_unique_id(uid))
    ctx.check(lib.rrte_hip_comm_init(ctx.h, 1, 0, uid))
    out = torch.full((w * h,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(lib.rrte_hip_render_gather_async(ctx.h, sc.ref(), C.byref(prm), 0, out.data_ptr(), None))
    ctx.check(lib.rrte_hip_flush(ctx.h))
    ctx.check(lib.rrte_hip_synchronize(ctx.h))
    assert ctx.accel_info().nodes > 0
    got = out.cpu().numpy().view(np.uint8)
    bad = got != plain
    assert not bad.any(), f"N={nranks}: {int(bad.sum())} bytes differ from the plain render"
    ctx.close()


def test_switching_the_policy_between_frames():
    w, h = 67, 37
    sc, prm = LoweredScene(mix(65, True), _lights(), cam_of(w, h)), cfg_of(w, h).lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    frames, nodes, bvh = [], [], []
    for policy in (OFF, ON, OFF, ON):
        ctx.set_scene_accel(policy, 1)
        _, lin, st = _render(ctx, sc, prm)
        frames.append((lin.copy(), int(st.shadow_rays)))
        nodes.append(ctx.accel_info().nodes)
        bvh.append(ctx.mesh_info().bvh_builds)
    assert nodes[0] == nodes[2] == 0 and nodes[1] == nodes[3] > 0
    # a switch uploads the scene again and builds the top level, but no mesh BVH (one per distinct range, once)
    assert ctx.accel_info().builds == 2 and bvh == [bvh[0]] * 4 and bvh[0] == ctx.mesh_info().ranges
    for lin, shadow in frames[1:]:
        assert np.array_equal(lin.view(np.uint32), frames[0][0].view(np.uint32)) and shadow == frames[0][1]
    ctx.close()


# ------------------------------------------------------------------------------ 7. it culls
def _sphere_bound(c, r):
    """sphere_bound of the host (rrte_amd/csrc/bvh.hip) for an untransformed sphere."""
    c = np.asarray(c, np.float64)
    r = r * 1.001 + 1e-3 + 1e-5 * np.abs(c).max()
    return np.array([*c.astype(F), np.nextafter(F(r), F(np.inf))], F)


def _camera_rays(cam, w, h):
    """Pixel-centre camera rays of the frame in float64: (origin (3,), directions (h, w, 3))."""
    sc = LoweredScene([], [], cam)
    ys, xs = (a.ravel() for a in np.mgrid[0:h, 0:w])
    rays = q.oracle_pick_rays(sc, w, h, xs, ys, 1e-3)
    d = rays["direction"].astype(np.float64).reshape(h, w, 3)
    return rays["origin"][0].astype(np.float64), d / np.linalg.norm(d, axis=2, keepdims=True)


def _rays_meet_box(o, d, lo, hi):
    """Slab test in float64 of rays (n, 3) from o against [lo, hi], t >= 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tn = np.nanmax(np.minimum(t0, t1), axis=1)
    tf = np.nanmin(np.maximum(t0, t1), axis=1)
    return tn <= np.maximum(tf, 0.0)


def test_it_culls(tmp_path):
    """256 small spheres on a 16x16 grid filling the view: the candidates the device counted lie between
    a lower bound (conservativeness at wave level: every object whose bounding sphere some pixel-centre
    ray of the tile meets is a candidate) and an upper bound (no more than the objects of the leaves
    whose box, enlarged by twice the documented inflation and slack, some ray of the tile meets)."""
    w, h = 64, 40
    cam = scenes._camera(w, h, (0.0, 0.0, 20.0), (0.0, 0.0, 0.0))
    centres = [(((i % 16) - 7.5) * 1.25, ((i // 16) - 7.5) * 0.78, 0.0) for i in range(256)]
    objs = [Sphere(c, 0.3, _mat(0.3 + 0.002 * i, 0.5, 0.7)) for i, c in enumerate(centres)]
    sc, prm = LoweredScene(objs, _lights(), cam), cfg_of(w, h, "refcompat").lower()
    ctx = accel_ctx(flags=abi.ACCEL_COUNT)
    _check_frame(ctx, sc, prm, _oracle_frame(("grid", w, h), sc, prm), False)
    a = ctx.accel_info()
    ctx.close()
    tiles = [(ty, tx) for ty in range(h // 8) for tx in range(w // 8)]
    assert a.searches == len(tiles) == 40  # every wave has a live pixel and walks once (depth 1, spp 1)
    bounds = np.stack([_sphere_bound(c, 0.3) for c in centres])
    head, leaves = dump(build_tool(tmp_path, sanitize=False), bounds)
    assert head[0] == "built" and int(head[2]) == a.nodes and int(head[3]) == a.depth
    o, d = _camera_rays(cam, w, h)
    lower = upper = 0
    for ty, tx in tiles:
        dt = d[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(-1, 3)
        # lower: ray meets the bounding sphere (|oc x d| <= r, in front)
        oc = bounds[:, None, :3].astype(np.float64) - o
        along = (oc * dt[None]).sum(2)
        perp2 = (oc * oc).sum(2) - along ** 2
        lower += int(((perp2 <= bounds[:, None, 3].astype(np.float64) ** 2) & (along > 0)).any(1).sum())
        for lo, hi, members in leaves:
            lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
            # twice §20's inflation and slack: the lane widening e = 2^-21 (max(|lo|, |hi|) + |o|) per axis
            # and the accept slack 2^-22 (|tn| + |tf|) <= 2^-21 * 64 in t for this scene (t < 32), as a
            # distance along a unit direction
            e = 2.0 * (2.0 ** -21 * (np.maximum(np.abs(lo64), np.abs(hi64)) + np.abs(o)) + 2.0 ** -21 * 64.0)
            if _rays_meet_box(o, dt, lo64 - e, hi64 + e).any():
                upper += len(members)
    print(f"candidates {a.candidates}: lower {lower}, upper {upper}, linear {256 * a.searches}")
    assert upper < 256 * a.searches / 4, "the scene does not test culling"
    assert lower <= a.candidates <= upper
