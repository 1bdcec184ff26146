"""Frame AOVs on the GPU (include/rrte_hip_aov.h: rrte_hip_render_aov / render_aov_async) against the
oracle loop (tests/aov_ref.py over query_ref.oracle_closest and query_ref.oracle_pick_rays; instance_ref's
checker where a scene holds mesh instances, which the C oracle does not know).  Every plane is compared
as uint32, a NaN on both sides counting as equal.  The reference is never a second run of the new code."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_ref as ar
import instance_ref as ir
import scenes_extra as se
from rrte_amd import (Color, LambertianMaterial, LoweredScene, MeshInstance, Raytracer, RaytracerConfig, Sphere,
                      Transform, abi, scenes)
from rrte_amd.mesh import icosphere, torus
from test_gpu_accel import cam_of, mix

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ATOOL = ROOT / "rrte_amd" / "lib" / "cpp_aov_tool"
W, H = 33, 19  # partial tiles on the right (33 = 4 * 8 + 1) and at the bottom (19 = 2 * 8 + 3)
SENTINEL = 0xA5
GUARD = 64  # elements before and after every output array

BUILDERS = {
    "sdf_showcase": lambda w, h: scenes.sdf_showcase(w, h),
    "mixed_scene": lambda w, h: se.mixed_scene(w, h, "lambert_shadow"),
    "ortho_scene": lambda w, h: se.ortho_scene(w, h, "lambert_shadow"),
    "deformers_scene": lambda w, h: se.deformers_scene(w, h, "lambert_shadow"),
    "mesh_demo": lambda w, h: scenes.mesh_demo(w, h, detail=0.3),
}
# (hits, misses) of the 33x19 reference views, counted on the CPU when the tests were written
COVERAGE = {"sdf_showcase": (448, 179), "mixed_scene": (547, 80), "ortho_scene": (138, 489),
            "mesh_demo": (522, 105), "deformers_scene": (495, 132)}


@functools.lru_cache(maxsize=None)
def scene_of(name, w=W, h=H):
    return BUILDERS[name](w, h)


@functools.lru_cache(maxsize=None)
def lowered(name, w=W, h=H):
    objs, lights, cam, _ = scene_of(name, w, h)
    return LoweredScene(objs, lights, cam)


@functools.lru_cache(maxsize=None)
def want_records(name, w=W, h=H):
    """The oracle loop's record of every pixel of the w x h view, computed once."""
    rec = ar.pick_records(lowered(name, w, h), w, h, scene_of(name, w, h)[3].t_min)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def want_planes(name, w=W, h=H):
    cfg = scene_of(name, w, h)[3]
    return ar.planes_of(lowered(name, w, h), want_records(name, w, h), list(cfg.lower().background), (h, w))


@functools.lru_cache(maxsize=None)
def want_mesh_tri(name):
    """TRI of the mesh pixels of the 33x19 view, which the C oracle cannot give: instance_ref's checker
    (the lowest triangle index whose own test reports the winning t) over every third of those pixels
    (it tests each of a mesh's triangles per pixel).  Returns (ys, xs, tri); the checker must name the C
    oracle's object for every one of them."""
    sc = lowered(name)
    ys, xs = (a[::3] for a in np.nonzero(ar.on_mesh(sc, want_planes(name)["prim"])))
    rec = ar.pick_records(sc, W, H, scene_of(name)[3].t_min, pixels=np.stack([xs, ys], axis=1), closest=ir.closest)
    assert np.array_equal(rec["prim"], want_planes(name)["prim"][ys, xs])
    return ys, xs, rec["tri"].astype("<u4")


def render_aov(rt, name, planes=abi.AOV_ALL, rect=None, w=W, h=H):
    objs, lights, cam, _ = scene_of(name, w, h)
    return rt.render_aov(objs, cam, planes, rect, lights=lights)


class RawPlanes:
    """One guarded, sentinel-filled array per plane for an n-pixel call of the C ABI: GUARD elements,
    the plane, GUARD elements.  `bufs(names)` points rrte_aov_buffers at the interiors of `names`."""

    def __init__(self, n):
        self.n = n
        self.arr = {}
        for name, (_, dtype, comps) in abi.AOV_PLANES.items():
            a = np.empty(2 * GUARD + n * max(comps, 1), dtype=dtype)
            a.view(np.uint8)[:] = SENTINEL
            self.arr[name] = a

    def bufs(self, names):
        b = abi.AovBuffers()
        for name in names:
            a = self.arr[name]
            setattr(b, name, C.cast(C.c_void_p(a.ctypes.data + GUARD * a.itemsize), type(getattr(b, name))))
        return b

    def interior(self, name, shape):
        comps = abi.AOV_PLANES[name][2]
        return self.arr[name][GUARD:len(self.arr[name]) - GUARD].reshape(shape + ((comps,) if comps else ()))

    def untouched(self, name):
        return bool((self.arr[name].view(np.uint8) == SENTINEL).all())

    def guards_intact(self, name):
        a = self.arr[name]
        return bool((a[:GUARD].view(np.uint8) == SENTINEL).all() and (a[len(a) - GUARD:].view(np.uint8) == SENTINEL).all())


def raw_call(rt, sc, prm, planes, rect, raw, names):
    x0, y0, w, h = rect
    desc = abi.AovDesc(planes=planes, x0=x0, y0=y0, width=w, height=h)
    bufs = raw.bufs(names)
    return rt.ctx.lib.rrte_hip_render_aov(rt.ctx.h, sc.ref(), C.byref(prm), C.byref(desc), C.byref(bufs))


# --------------------------------------------------------------- 1. every plane, whole frame
@pytest.mark.parametrize("name", list(BUILDERS))
def test_every_plane_of_the_whole_frame(name):
    rec, want = want_records(name), want_planes(name)
    sc = lowered(name)
    hit = rec["prim"] >= 0
    hits, misses = int(hit.sum()), int((~hit).sum())
    kinds = {int(sc.prims[int(p)].kind) for p in set(rec["prim"][hit])}
    back = int((hit & (rec["front_face"] == 0)).sum())
    print(name, "oracle: hits", hits, "misses", misses, "distinct objects", len(set(rec["prim"][hit])), "kinds",
          sorted(kinds), "back-face hits", back)
    # no view passes vacuously
    assert (hits, misses) == COVERAGE[name]
    if name == "sdf_showcase":
        assert len(set(rec["prim"][hit])) == 17
    if name == "mixed_scene":
        assert set(range(1, 7)) <= kinds and back == 12
    if name == "ortho_scene":
        assert back == 16
    got = render_aov(Raytracer(scene_of(name)[3], device=0), name)
    assert set(got) == set(ar.PLANES)
    # the C oracle has no triangle index: TRI of mesh pixels comes from instance_ref's checker
    mesh_px = ar.on_mesh(sc, want["prim"])
    ar.assert_planes_equal(got, want, skip_tri=mesh_px)
    assert not got["tri"][~mesh_px].any()
    assert mesh_px.any() == (name == "mesh_demo")
    if mesh_px.any():
        ys, xs, tri = want_mesh_tri(name)
        assert len(tri) >= 60 and len(set(tri)) >= 50
        assert np.array_equal(got["tri"][ys, xs], tri)
    assert (got["normal"][..., 3] == 0).any() == (back > 0 or misses > 0)


@pytest.mark.parametrize("name", ["sdf_showcase", "ortho_scene"])
def test_a_one_pixel_frame(name):
    """A 1x1 frame: one live lane and 63 idle ones."""
    got = render_aov(Raytracer(scene_of(name, 1, 1)[3], device=0), name, w=1, h=1)
    want = want_planes(name, 1, 1)
    assert got["depth"].shape == (1, 1) and got["normal"].shape == (1, 1, 4)
    ar.assert_planes_equal(got, want)


# --------------------------------------------------------------- 2. rectangles
RECTS = [(3, 5, 11, 9), (0, 0, 33, 19), (32, 18, 1, 1), (25, 0, 8, 19), (0, 11, 33, 8), (7, 7, 9, 9)]


@pytest.mark.parametrize("name", ["sdf_showcase", "mixed_scene"])
def test_rectangles_are_sub_blocks_of_the_frame(name):
    sc, prm, want = lowered(name), scene_of(name)[3].lower(), want_planes(name)
    mesh_px = ar.on_mesh(sc, want["prim"])
    if name == "sdf_showcase":  # the first rectangle holds hits and misses
        blk = ar.sub_block(want, RECTS[0])["prim"]
        assert (int((blk >= 0).sum()), int((blk < 0).sum())) == (95, 4)
    rt = Raytracer(scene_of(name)[3], device=0)
    for rect in RECTS:
        x0, y0, w, h = rect
        raw = RawPlanes(w * h)
        assert raw_call(rt, sc, prm, abi.AOV_ALL, rect, raw, ar.PLANES) == abi.RRTE_OK, rect
        got = {n: raw.interior(n, (h, w)) for n in ar.PLANES}
        ar.assert_planes_equal(got, ar.sub_block(want, rect), skip_tri=mesh_px[y0:y0 + h, x0:x0 + w])
        for n in ar.PLANES:
            assert raw.guards_intact(n), (rect, n)
    # the Python wrapper's rect; the all-zero rectangle given as a value is the whole frame, as in the header
    ar.assert_planes_equal(render_aov(rt, name, rect=RECTS[0]), ar.sub_block(want, RECTS[0]), skip_tri=mesh_px[5:14, 3:14])
    whole = render_aov(rt, name, rect=(0, 0, 0, 0))
    assert whole["depth"].shape == (H, W) and whole["normal"].shape == (H, W, 4)
    ar.assert_planes_equal(whole, want, skip_tri=mesh_px)


# --------------------------------------------------------------- 3. plane subsets
def test_plane_subsets_leave_the_other_arrays_alone():
    name = "mixed_scene"
    sc, prm, want = lowered(name), scene_of(name)[3].lower(), want_planes(name)
    rt = Raytracer(scene_of(name)[3], device=0)
    for mask in (abi.AOV_DEPTH | abi.AOV_PRIM, abi.AOV_NORMAL, abi.AOV_ALL):
        asked = [n for n in ar.PLANES if abi.AOV_PLANES[n][0] & mask]
        raw = RawPlanes(W * H)
        # every array is handed over, requested or not
        assert raw_call(rt, sc, prm, mask, (0, 0, 0, 0), raw, ar.PLANES) == abi.RRTE_OK
        got = {n: raw.interior(n, (H, W)) for n in asked}
        ar.assert_planes_equal(got, want, names=asked, skip_tri=ar.on_mesh(sc, want["prim"]))
        for n in ar.PLANES:
            assert raw.guards_intact(n), n
            if n not in asked:
                assert raw.untouched(n), (hex(mask), n)
        # and the wrapper returns exactly the planes asked for
        assert list(render_aov(rt, name, planes=asked)) == asked


# --------------------------------------------------------------- 4. TRI
def _two_meshes():
    mat = LambertianMaterial(Color.rgb(0.7, 0.5, 0.3))
    ground = Sphere((0, -1000, 0), 1000, LambertianMaterial(Color.rgb(0.3, 0.3, 0.3)))
    return ground, mat


def _view(objs, cam, cfg, planes=abi.AOV_ALL):
    return Raytracer(cfg, device=0).render_aov(objs, cam, planes)


def test_triangle_index():
    """test_gpu_query.test_mesh_triangle_index's two small meshes as a view: lowered as meshes and
    triangle by triangle, the same planes bit for bit, and TRI names the triangle that wins in the
    second form."""
    ground, mat = _two_meshes()
    meshes = [icosphere((-1.2, 1.0, 0.0), 0.9, 2, mat), torus((1.3, 1.0, 0.0), 0.8, 0.3, 16, 8, mat)]
    cam = scenes._camera(W, H, (0.0, 1.8, 3.4), (0.0, 0.95, 0.0))
    cfg = RaytracerConfig(width=W, height=H)
    am = _view([ground] + meshes, cam, cfg)
    at = _view([ground] + [t for m in meshes for t in m.triangles()], cam, cfg)
    first = np.cumsum([1] + [m.num_triangles for m in meshes])  # object index of each mesh's first triangle
    on_mesh = am["prim"] >= 1
    assert on_mesh.sum() >= 100 and set(am["prim"][on_mesh]) == {1, 2} and (am["prim"] == 0).any()
    assert len(set(am["tri"][on_mesh])) >= 50
    assert np.array_equal(first[am["prim"][on_mesh] - 1] + am["tri"][on_mesh], at["prim"][on_mesh])
    assert np.array_equal(am["prim"][~on_mesh], at["prim"][~on_mesh])
    assert not am["tri"][~on_mesh].any() and not at["tri"].any()
    ar.assert_planes_equal(am, at, names=["depth", "material", "normal", "position", "albedo"])


def test_triangle_index_with_an_instance():
    """The same with the icosphere placed as a MeshInstance: the torus against its triangle-by-triangle
    form, the instance (the same object in both forms) equal between them, and every plane, TRI
    included, against the checker that knows instances."""
    ground, mat = _two_meshes()
    base = icosphere((0.0, 0.0, 0.0), 0.9, 2, mat)
    inst = MeshInstance(base, Transform((-1.2, 1.0, 0.0), scenes.Q_Y45, (1.0, 0.8, 1.1)), mat)
    tor = torus((1.3, 1.0, 0.0), 0.8, 0.3, 16, 8, mat)
    cam = scenes._camera(W, H, (0.0, 1.8, 3.4), (0.0, 0.95, 0.0))
    cfg = RaytracerConfig(width=W, height=H)
    objs = [ground, inst, tor]
    am = _view(objs, cam, cfg)
    at = _view([ground, inst] + tor.triangles(), cam, cfg)
    on_inst, on_tor = am["prim"] == 1, am["prim"] == 2
    assert on_inst.sum() >= 40 and on_tor.sum() >= 40 and len(set(am["tri"][on_inst])) >= 20
    assert np.array_equal(2 + am["tri"][on_tor], at["prim"][on_tor])
    assert np.array_equal(am["prim"][~on_tor], at["prim"][~on_tor])
    assert np.array_equal(am["tri"][on_inst], at["tri"][on_inst]) and not am["tri"][am["prim"] <= 0].any()
    ar.assert_planes_equal(am, at, names=["depth", "material", "normal", "position", "albedo"])
    sc = LoweredScene(objs, [], cam)
    rec = ar.pick_records(sc, W, H, cfg.t_min, closest=ir.closest)
    ar.assert_planes_equal(am, ar.planes_of(sc, rec, list(cfg.lower().background), (H, W)))


# --------------------------------------------------------------- 5. the scene accelerator
def test_the_accelerator_changes_no_plane():
    objs, cam = mix(65, True), cam_of(W, H)
    cfg = RaytracerConfig(width=W, height=H)
    sc = LoweredScene(objs, [], cam)
    assert sc.ir.num_prims == 65 and any(p.kind == abi.PRIM_MESH_INSTANCE for p in sc.prims[:65])
    rec = ar.pick_records(sc, W, H, cfg.t_min, closest=ir.closest)
    want = ar.planes_of(sc, rec, list(cfg.lower().background), (H, W))
    assert len({int(p) for p in rec["prim"]}) >= 50
    on = Raytracer(cfg, device=0, jit=abi.JIT_OFF)
    on.ctx.set_scene_accel(abi.SCENE_ACCEL_ON, 1, abi.ACCEL_COUNT)
    off = Raytracer(cfg, device=0, jit=abi.JIT_OFF)
    a_on, a_off = on.render_aov(objs, cam), off.render_aov(objs, cam)
    # the AOV launch itself walked the tree: one walk per wave, one wave per 8x8 tile (5 x 3 of them)
    info = on.ctx.accel_info()
    assert info.nodes > 0 and info.searches == 5 * 3 and 0 < info.candidates <= 65 * info.searches
    assert off.ctx.accel_info().nodes == 0
    ar.assert_planes_equal(a_on, a_off)
    ar.assert_planes_equal(a_on, want)
    # a rectangle with partial tiles through the accelerated kernel: 11 x 9 pixels, 2 x 2 tiles
    ar.assert_planes_equal(on.render_aov(objs, cam, rect=RECTS[0]), ar.sub_block(want, RECTS[0]))
    assert on.ctx.accel_info().searches == 2 * 2
    on.ctx.close()
    off.ctx.close()


# --------------------------------------------------------------- 6. more than one staging chunk
def _four_spheres():
    m = [LambertianMaterial(Color.rgb(*c)) for c in ((0.5, 0.5, 0.5), (0.8, 0.2, 0.2), (0.2, 0.8, 0.2), (0.2, 0.2, 0.8))]
    return [Sphere((0.0, -1000.0, 0.0), 1000.0, m[0]), Sphere((-2.2, 1.0, 0.0), 1.0, m[1]),
            Sphere((0.0, 1.0, -1.0), 1.0, m[2]), Sphere((2.2, 1.0, 0.0), 1.0, m[3])]


def _check_pixels(got, sc, w, h, t_min, pixels):
    rec = ar.pick_records(sc, w, h, t_min, pixels=pixels)
    xs, ys = np.asarray(pixels).T
    want = ar.planes_of(sc, rec, [0.0] * 4)
    ar.assert_planes_equal({n: got[n][ys, xs] for n in ("depth", "prim")}, want, names=["depth", "prim"])
    return rec


def test_a_frame_larger_than_one_staging_chunk():
    """2049 x 2049 in one blocking call: the rows are staged in chunks of whole tile rows of at most
    2^22 pixels (255 tile rows of 2049 pixels: 2040 rows, then 9)."""
    w = h = 2049
    chunk_rows = 8 * ((1 << 22) // (8 * w))
    assert 0 < chunk_rows < h and chunk_rows % 8 == 0
    objs = _four_spheres()
    cam = scenes._camera(w, h, (0.0, 2.5, 8.0), (0.0, 0.8, 0.0))
    cfg = RaytracerConfig(width=w, height=h)
    got = Raytracer(cfg, device=0).render_aov(objs, cam, abi.AOV_DEPTH | abi.AOV_PRIM)
    assert list(got) == ["depth", "prim"] and got["prim"].shape == (h, w)
    px = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    rng = np.random.default_rng(0xA07)
    for b in range(chunk_rows, h, chunk_rows):  # two rows on each side of every chunk boundary
        px += [(int(x), y) for y in (b - 2, b - 1, b, b + 1) for x in rng.integers(0, w, 32)]
    px += [(int(x), int(y)) for x, y in zip(rng.integers(0, w, 512 - len(px)), rng.integers(0, h, 512 - len(px)))]
    assert len(px) == 512
    rec = _check_pixels(got, LoweredScene(objs, [], cam), w, h, cfg.t_min, px)
    assert len(set(rec["prim"])) >= 3 and (rec["prim"] < 0).any()
    # every pixel was written: a miss is -1 / +inf, a hit a valid index
    assert ((got["prim"] >= -1) & (got["prim"] < 4)).all() and (np.isinf(got["depth"]) == (got["prim"] < 0)).all()


def test_a_row_wider_than_one_staging_chunk():
    """One row of 2^19 + 9 pixels: wider than 2^22 / 8, so the row is staged in two column blocks."""
    w, h = (1 << 19) + 9, 1
    objs = _four_spheres()
    cam = scenes._camera(16, 9, (0.0, 2.5, 8.0), (0.0, 0.8, 0.0))  # a 16:9 view swept over the one long row
    cfg = RaytracerConfig(width=w, height=h)
    got = Raytracer(cfg, device=0).render_aov(objs, cam, abi.AOV_DEPTH | abi.AOV_PRIM)
    edge = 1 << 19
    rng = np.random.default_rng(0xA08)
    px = [(x, 0) for x in (0, 1, edge - 2, edge - 1, edge, edge + 1, w - 2, w - 1)] + [(int(x), 0) for x in rng.integers(0, w, 56)]
    rec = _check_pixels(got, LoweredScene(objs, [], cam), w, h, cfg.t_min, px)
    assert len(set(rec["prim"])) == 4
    assert ((got["prim"] >= -1) & (got["prim"] < 4)).all()


# --------------------------------------------------------------- 7. the async form
def test_async_form_matches_blocking():
    import torch
    name = "mixed_scene"
    objs, lights, cam, cfg = scene_of(name)
    rt = Raytracer(cfg, device=0)
    rect = (3, 5, 11, 9)
    for r in (None, rect):
        w, h = (W, H) if r is None else r[2:]
        want = render_aov(rt, name, rect=r)
        dev = {n: torch.full(((w * h * max(abi.AOV_PLANES[n][2], 1) + 2 * GUARD) * 4,), SENTINEL, dtype=torch.uint8,
                             device="cuda") for n in ar.PLANES}
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        addr = {n: t.data_ptr() + GUARD * 4 for n, t in dev.items()}
        assert all(a % 16 == 0 for a in addr.values())
        rt.render_aov_async(objs, cam, abi.AOV_ALL, addr, rect=r, stream=C.c_void_p(stream.cuda_stream), lights=lights)
        stream.synchronize()
        for n, t in dev.items():
            out = t.cpu().numpy()
            assert (out[:GUARD * 4] == SENTINEL).all() and (out[len(out) - GUARD * 4:] == SENTINEL).all(), n
            assert out[GUARD * 4:len(out) - GUARD * 4].tobytes() == want[n].tobytes(), n
    ar.assert_planes_equal(want, ar.sub_block(want_planes(name), rect), skip_tri=ar.on_mesh(lowered(name), want["prim"]))
    # a float[4] plane that is not 16-byte aligned, a 4-byte plane that is not 4-byte aligned
    with pytest.raises(abi.RrteError) as e:
        rt.render_aov_async(objs, cam, abi.AOV_NORMAL, {"normal": addr["normal"] + 4}, lights=lights)
    assert e.value.status == abi.RRTE_INVALID_ARG
    with pytest.raises(abi.RrteError) as e:
        rt.render_aov_async(objs, cam, abi.AOV_DEPTH, {"depth": addr["depth"] + 2}, lights=lights)
    assert e.value.status == abi.RRTE_INVALID_ARG
    rt.render_aov_async(objs, cam, abi.AOV_DEPTH, {"depth": addr["depth"] + 4}, rect=rect, lights=lights)  # 4-byte aligned
    rt.ctx.check(rt.ctx.lib.rrte_hip_synchronize(rt.ctx.h))
    assert rt.stats().frames == 0


# --------------------------------------------------------------- 8. coexistence with rendering
@pytest.mark.parametrize("jit", [abi.JIT_OFF, abi.JIT_ON])
def test_aovs_coexist_with_rendering(jit):
    """render, AOV, render with one Raytracer: both frames are a fresh context's frame, the statistics
    those of the renders alone, and the AOV's misses are the frame's background pixels."""
    name = "sdf_showcase"
    objs, lights, cam, cfg = scene_of(name)
    assert (cfg.jitter, cfg.samples_per_pixel, cfg.mode) == ("center", 1, "lambert_shadow")
    fresh = Raytracer(cfg, device=0, jit=jit)
    want8, wantf = fresh.render_f32(objs, lights, [], cam, linear=True)
    ws = fresh.stats()
    rt = Raytracer(cfg, device=0, jit=jit)
    a8, af = rt.render_f32(objs, lights, [], cam, linear=True)
    s1 = rt.stats()
    aov = rt.render_aov(objs, cam, lights=lights)
    s2 = rt.stats()
    b8, bf = rt.render_f32(objs, lights, [], cam, linear=True)
    s3 = rt.stats()
    for g8, gf in ((a8, af), (b8, bf)):
        assert np.array_equal(g8, want8) and np.array_equal(gf.view(np.uint32), wantf.view(np.uint32))
    for s in (s1, s2, s3):
        assert (s.primary_rays, s.shadow_rays) == (ws.primary_rays, ws.shadow_rays)
        assert s.jit_active == (1 if jit == abi.JIT_ON else 0)
    assert (s1.frames, s2.frames, s3.frames) == (1, 1, 2)
    assert s3.upload_ms == 0.0  # the scene stayed cached across the AOV call
    # the AOV's rays are the frame's rays: a miss exactly where the linear frame is the background
    # (r, g, b: the pixel sum starts from BLACK, whose alpha of 1 is added to the background's)
    bg = np.array(list(cfg.lower().background), np.float32)[:3]
    is_bg = (af.reshape(H, W, 4)[..., :3].view(np.uint32) == bg.view(np.uint32)).all(axis=2)
    assert 0 < is_bg.sum() < is_bg.size
    assert np.array_equal(aov["prim"] == -1, is_bg)
    ar.assert_planes_equal(aov, want_planes(name), skip_tri=ar.on_mesh(lowered(name), aov["prim"]))


# --------------------------------------------------------------- 9. error paths
def test_error_paths_leave_the_context_usable():
    name = "sdf_showcase"
    sc, cfg = lowered(name), scene_of(name)[3]
    prm = cfg.lower()
    rt = Raytracer(cfg, device=0)
    lib, h = rt.ctx.lib, rt.ctx.h
    raw = RawPlanes(W * H)
    full = raw.bufs(ar.PLANES)

    def call(scene=sc.ref(), params=prm, desc=None, bufs=full, **kw):
        d = abi.AovDesc(planes=abi.AOV_ALL, **kw) if desc is None else desc
        return lib.rrte_hip_render_aov(h, scene, C.byref(params) if params is not None else None,
                                       C.byref(d) if d is not False else None, C.byref(bufs) if bufs is not None else None)

    def desc(**kw):
        return abi.AovDesc(**{"planes": abi.AOV_ALL, **kw})

    padded = desc()
    padded._pad[1] = 1
    reserved = raw.bufs(ar.PLANES)
    reserved._reserved = 8
    huge = abi.RenderParams.from_buffer_copy(prm)
    huge.width, huge.height = 1 << 16, (1 << 14) + 1  # more than 2^30 pixels
    empty = abi.RenderParams.from_buffer_copy(prm)
    empty.width = 0
    big = 0xFFFFFFFF
    bad = {
        "null scene": call(scene=None), "null params": call(params=None), "null desc": call(desc=False),
        "null buffers": call(bufs=None),
        "no plane": call(desc=desc(planes=0)), "unknown bit": call(desc=desc(planes=0x80)),
        "unknown high bit": call(desc=desc(planes=0x80000001)),
        "null requested plane": call(bufs=raw.bufs(["depth", "prim"])),
        "null requested plane 2": call(desc=desc(planes=abi.AOV_NORMAL), bufs=raw.bufs(["depth"])),
        "pad": call(desc=padded), "reserved": call(bufs=reserved),
        "empty width": call(x0=1, y0=1, width=0, height=4), "empty height": call(x0=1, y0=1, width=4, height=0),
        "zero size off origin": call(x0=1, y0=0, width=0, height=0),
        "x0 outside": call(x0=W, y0=0, width=1, height=1), "y0 outside": call(x0=0, y0=H, width=1, height=1),
        "too wide": call(x0=1, y0=0, width=W, height=1), "too tall": call(x0=0, y0=1, width=1, height=H),
        "x sum wraps": call(x0=2, y0=0, width=big - 1, height=1), "y sum wraps": call(x0=0, y0=2, width=1, height=big - 1),
        "x0 wraps": call(x0=big, y0=0, width=2, height=1),
        "frame too large": call(params=huge, x0=0, y0=0, width=1, height=1), "empty frame": call(params=empty),
    }
    assert bad == {k: abi.RRTE_INVALID_ARG for k in bad}
    assert lib.rrte_hip_last_error(h)
    d1 = desc()
    assert lib.rrte_hip_render_aov(None, sc.ref(), C.byref(prm), C.byref(d1), C.byref(full)) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_render_aov_async(h, sc.ref(), C.byref(prm), C.byref(d1), None, None) == abi.RRTE_INVALID_ARG
    # a malformed SDF program: refused by the scene's validation
    objs, lights, cam, _ = scene_of(name)
    broken = LoweredScene(objs, lights, cam)
    first = next(p.sdf_first for p in broken.prims if p.kind == abi.PRIM_SDF)
    broken.nodes[first].op = abi.SDF_UNION
    assert call(scene=broken.ref()) == abi.RRTE_INVALID_ARG
    assert b"malformed SDF program" in lib.rrte_hip_last_error(h)
    for n in ar.PLANES:
        assert raw.untouched(n), n  # nothing was written
    # the next valid call on the same context succeeds, and a plane that is not requested may be null
    assert call(desc=desc(planes=abi.AOV_DEPTH | abi.AOV_PRIM), bufs=raw.bufs(["depth", "prim"])) == abi.RRTE_OK
    got = {n: raw.interior(n, (H, W)) for n in ("depth", "prim")}
    ar.assert_planes_equal(got, want_planes(name), names=["depth", "prim"])
    assert rt.stats().frames == 0


# --------------------------------------------------------------- 10. mirrors
def test_cpp_mirror_matches_python(tmp_path):
    subprocess.run(["make", "-s", "-C", str(ROOT / "rrte_amd" / "cpp")], check=True)
    objs, lights, cam, cfg = scenes.sdf_showcase(W, H)
    rt = Raytracer(cfg, device=0)
    for mask, rect in ((abi.AOV_ALL, (0, 0, 0, 0)), (abi.AOV_DEPTH | abi.AOV_NORMAL | abi.AOV_ALBEDO, (3, 5, 11, 9))):
        out = tmp_path / f"aov_{mask}.bin"
        r = subprocess.run([str(ATOOL), "aov", "sdf-showcase", str(W), str(H), hex(mask), *map(str, rect), str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        w, h = (W, H) if not any(rect) else rect[2:]
        assert f"aov {w}x{h} planes {hex(mask)} frames 0" in r.stdout
        want = rt.render_aov(objs, cam, mask, rect if any(rect) else None, lights=lights)
        assert out.read_bytes() == b"".join(want[n].tobytes() for n in ar.PLANES if n in want)
