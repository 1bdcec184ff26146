"""Mesh instances (RRTE_PRIM_MESH_INSTANCE, include/rrte_hip.h) on the device, against the CPU checker
tests/instance_ref.py: ray queries bit for bit on every field, frames (generic, full and topology
kernels) with the linear image and the shadow-ray count identical, one BVH per distinct range, no BVH
build when only transforms or other objects change, kind 8 unchanged, the emulated multi-GPU peers,
argument errors and the RRTE_DEBUG=4 check word."""
import ctypes as C

import numpy as np
import pytest

import instance_ref as ir
import query_ref as q
from rrte_amd import (Camera, Color, Cube, LambertianMaterial, LoweredScene, MeshInstance, PointLight, Raytracer,
                      RaytracerConfig, SDFObject, SDFSphere, Sphere, Transform, abi, scenes)
from rrte_amd.mesh import icosphere
from rrte_amd.renderer import Context

pytestmark = pytest.mark.gpu

DETAIL = 0.1  # instance_demo's smallest meshes: 320 + 256 triangles


def _mat(r, g, b):
    return LambertianMaterial(Color.rgb(r, g, b))


def _lights():
    return [PointLight((-10.0, 15.0, 10.0), Color.rgb(1.0, 1.0, 1.0), 25.0),
            PointLight((10.0, 10.0, 15.0), Color.rgb(0.6, 0.7, 1.0), 15.0)]


def scene_a():
    """One instance of icosphere(1) under a rotated, non-uniformly scaled transform (large enough for
    the generator's rays to hit it often)."""
    ball = icosphere((0.0, 1.0, 0.0), 1.0, 1, _mat(0.8, 0.3, 0.3))
    return [MeshInstance(ball, Transform((0.5, 1.0, -1.0), scenes.Q_X45_Y45, (5.0, 2.0, 4.0)))]


def scene_b():
    """Ground sphere, the base as a plain mesh, two instances of it (one mirrored), a cube, and an SDF
    sphere AFTER them in the list, so its t_max is narrowed by instance hits."""
    ball = icosphere((0.0, 1.5, 0.0), 1.5, 1, _mat(0.8, 0.3, 0.3))
    cube = Cube((4.0, 1.0, -3.0), (2.0, 2.0, 2.0), _mat(0.3, 0.8, 0.3))
    cube.set_transform(Transform((0.0, 0.0, 0.0), scenes.Q_Y45, (1.0, 1.0, 1.0)))
    return [Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.5, 0.5, 0.5)), ball,
            MeshInstance(ball, Transform((-4.0, 0.5, 2.0), scenes.Q_Y45, (1.5, 0.8, 1.2)), _mat(0.2, 0.4, 0.9)),
            MeshInstance(ball, Transform((4.5, 0.0, 3.0), scenes.Q_X45, (-1.2, 1.0, 1.0))),
            cube, SDFObject(SDFSphere((-1.0, 1.5, 4.5), 2.0), _mat(0.9, 0.9, 0.2))]


QUERY_SCENES = {"a": scene_a, "b": scene_b}


# ---------------------------------------------------------------------------------- 6. queries
@pytest.mark.parametrize("any_hit", [False, True])
@pytest.mark.parametrize("name", list(QUERY_SCENES))
def test_queries_match_the_checker_bit_for_bit(name, any_hit):
    objs = QUERY_SCENES[name]()
    o, d, length = q.gen_rays()
    # every third ray is a segment that stops short of its target, the others run to infinity
    t_max = np.where(np.arange(len(o)) % 3 == 0, length * np.float32(0.8), q.INF).astype(np.float32)
    rays = q.rays_of(o, d, q.T_MIN, t_max)
    got = Raytracer(device=0).raycast(objs, o, d, q.T_MIN, t_max, any_hit=any_hit)
    sc = LoweredScene(objs, [], Camera())
    want = ir.any_hit(sc, rays) if any_hit else ir.closest(sc, rays)
    assert (want["prim"] >= 0).sum() > 40, "the rays hardly touch the scene"
    on_instance = sum(sc.prims[i].kind == abi.PRIM_MESH_INSTANCE for i in want["prim"][want["prim"] >= 0])
    assert on_instance >= 10, "the rays hardly touch an instance"
    q.assert_hits_equal(got, want, tri=True)


def test_pick_matches_the_checker():
    w, h = 64, 36
    objs = scene_b()
    cam = scenes._camera(w, h, (0.0, 6.0, 14.0), (0.0, 1.0, 0.0))
    xs = np.array([5, 16, 24, 32, 40, 48, 58, 20, 44])
    ys = np.array([30, 18, 20, 17, 19, 21, 5, 26, 14])
    rt = Raytracer(RaytracerConfig(width=w, height=h), device=0)
    got = rt.pick(objs, cam, xs, ys)
    sc = LoweredScene(objs, [], cam)
    want = ir.closest(sc, q.oracle_pick_rays(sc, w, h, xs, ys, rt.config.t_min))
    assert len({int(p) for p in want["prim"]}) >= 3
    q.assert_hits_equal(got, want, tri=True)


# ----------------------------------------------------------------------------------- 7. frames
def _render(ctx, sc, prm, linear=True):
    p = abi.RenderParams.from_buffer_copy(prm)
    if linear:
        p.flags |= abi.FLAG_F32_LINEAR
    n = p.width * p.height * 4
    out8, outf = np.empty(n, np.uint8), np.empty(n, np.float32)
    ctx.check(ctx.lib.rrte_hip_render_f32(ctx.h, sc.ref(), C.byref(p), out8.ctypes.data, outf.ctypes.data))
    return out8, outf, ctx.stats()


_want = {}


def _reference(monkeypatch, key, sc, prm):
    """The checker's frame of a scene, computed once per key: (rgba8, linear f32, shadow rays)."""
    if key not in _want:
        r8, _, _ = ir.render(monkeypatch, sc, prm, linear=False)
        _, lin, shadow = ir.render(monkeypatch, sc, prm, linear=True)
        for a in (r8, lin):
            a.setflags(write=False)
        _want[key] = (r8.reshape(-1), lin.reshape(-1), shadow)
    return _want[key]


def _check_frame(ctx, sc, prm, want, expect_jit):
    r8, lin, shadow = want
    g8, glin, st = _render(ctx, sc, prm)
    assert st.jit_active == expect_jit
    bad = np.flatnonzero(glin.view(np.uint32) != lin.view(np.uint32))
    assert bad.size == 0, (bad[:8] // 4, glin[bad[:8]], lin[bad[:8]])
    assert int(st.shadow_rays) == shadow
    g8, _, _ = _render(ctx, sc, prm, linear=False)
    assert np.abs(g8.astype(np.int16) - r8.astype(np.int16)).max() <= 1


VARIANTS = {"generic": (abi.JIT_OFF, None, 0), "full": (abi.JIT_ON, "0", 1), "topology": (abi.JIT_ON, "1", 2)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
@pytest.mark.parametrize("w,h", [(64, 36), (67, 37)])
def test_instance_demo_frames(w, h, mode, variant, monkeypatch):
    jit, topo, expect = VARIANTS[variant]
    if topo is None:
        monkeypatch.delenv("RRTE_JIT_TOPO", raising=False)
    else:
        monkeypatch.setenv("RRTE_JIT_TOPO", topo)
    objs, lights, cam, cfg = scenes.instance_demo(w, h, mode, detail=DETAIL)
    assert cfg.max_depth == 1 and len(lights) == 2
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    want = _reference(monkeypatch, ("demo", w, h, mode), sc, prm)
    ctx = Context(0, jit=jit)
    _check_frame(ctx, sc, prm, want, expect)
    ctx.close()


def thin_scene(w, h):
    """A long thin instance -- scale (4, 0.3, 0.3), rotated 45 degrees about two axes -- crossing many
    tiles: a culling bound built from the wrong scale would clip it."""
    ball = icosphere((0.0, 0.0, 0.0), 1.0, 1, _mat(0.8, 0.5, 0.2))
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.4, 0.4, 0.4)),
            MeshInstance(ball, Transform((0.0, 2.5, 0.0), scenes.Q_X45_Y45, (4.0, 0.3, 0.3)))]
    cam = scenes._camera(w, h, (0.0, 4.0, 9.0), (0.0, 2.0, 0.0))
    cfg = RaytracerConfig(max_depth=1, samples_per_pixel=1, width=w, height=h, mode="lambert_shadow", jitter="center")
    return objs, _lights(), cam, cfg


@pytest.mark.parametrize("tile_cull", ["1", "0"])
def test_long_thin_instance_is_not_clipped(tile_cull, monkeypatch):
    w, h = 64, 36
    objs, lights, cam, cfg = thin_scene(w, h)
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    want = _reference(monkeypatch, ("thin", w, h), sc, prm)
    # the instance really spans many 8x8 tiles in the checker's frame
    lin = want[1].reshape(h, w, 4)
    ground_only = ir.render(monkeypatch, LoweredScene(objs[:1], lights, cam), prm)[1]
    cover = (lin.view(np.uint32) != ground_only.view(np.uint32)).any(axis=2)
    tiles = {(y // 8, x // 8) for y, x in zip(*np.nonzero(cover))}
    assert len(tiles) >= 8 and len({x for _, x in tiles}) >= 4
    monkeypatch.setenv("RRTE_TILE_CULL", tile_cull)
    ctx = Context(0, jit=abi.JIT_OFF)
    _check_frame(ctx, sc, prm, want, 0)
    ctx.close()


# ------------------------------------------------------------------------ 8. sharing and cache
def _family(w, h):
    ball = icosphere((0.0, 1.0, 0.0), 1.0, 2, _mat(0.8, 0.3, 0.3))
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.5, 0.5, 0.5)), ball,
            MeshInstance(ball, Transform((-3.0, 0.0, 0.5), scenes.Q_Y90, (1.0, 1.0, 1.0))),
            MeshInstance(ball, Transform((3.0, 0.2, 0.0), scenes.Q_X45, (0.7, 1.4, 0.7)), _mat(0.3, 0.7, 0.4)),
            MeshInstance(ball, Transform((0.5, 0.0, 3.0), scenes.Q_Y45, (-0.6, 0.6, 0.6))),
            Sphere((-1.5, 0.6, 3.5), 0.6, _mat(0.9, 0.8, 0.2))]
    cam = scenes._camera(w, h, (0.0, 5.0, 11.0), (0.0, 1.0, 0.0))
    cfg = RaytracerConfig(max_depth=1, samples_per_pixel=1, width=w, height=h, mode="lambert_shadow", jitter="center")
    return ball, objs, _lights(), cam, cfg


def test_one_bvh_per_range_and_none_for_a_transform_change(monkeypatch):
    monkeypatch.setenv("RRTE_JIT_TOPO", "1")
    w, h = 64, 36
    ball, objs, lights, cam, cfg = _family(w, h)
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    assert [sc.prims[i].kind for i in range(6)] == [0, 8, 9, 9, 9, 0]
    ctx = Context(0, jit=abi.JIT_ON)
    _check_frame(ctx, sc, prm, _reference(monkeypatch, ("family", 0), sc, prm), 2)
    mi = ctx.mesh_info()
    assert (mi.ranges, mi.bvh_builds, mi.tri_slots) == (1, 1, ball.num_triangles)
    assert mi.bvh_nodes > 0
    # the same arrays and ranges: one instance turns and grows, and an unrelated sphere moves
    sc.prims[3].trs[:] = [2.5, 0.6, -0.5, *scenes.Q_X45_Y45, 1.1, 0.9, 1.3]
    sc.prims[5].p[0], sc.prims[5].p[2] = 1.5, 4.0
    _check_frame(ctx, sc, prm, _reference(monkeypatch, ("family", 1), sc, prm), 2)
    mi = ctx.mesh_info()
    assert (mi.ranges, mi.bvh_builds, mi.tri_slots) == (1, 1, ball.num_triangles)
    _, moved, _ = _render(ctx, sc, prm)
    fresh_ctx = Context(0, jit=abi.JIT_ON)
    _, fresh, st = _render(fresh_ctx, sc, prm)
    assert np.array_equal(moved.view(np.uint32), fresh.view(np.uint32))
    assert fresh_ctx.mesh_info().bvh_builds == 1
    # another set of ranges (one triangle less in a second range) does build: two ranges, three builds so far
    sc.prims[4].sdf_count -= 1
    _render(ctx, sc, prm)
    mi = ctx.mesh_info()
    assert (mi.ranges, mi.bvh_builds, mi.tri_slots) == (2, 3, 2 * ball.num_triangles - 1)
    fresh_ctx.close()
    ctx.close()


# ------------------------------------------------------------------------- 9. kind 8 unchanged
def test_two_plain_meshes_naming_one_range():
    from test_gpu_parity import compare
    w, h = 96, 54
    ball = icosphere((0.0, 1.2, 0.0), 1.2, 2, _mat(0.8, 0.3, 0.3))
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.5, 0.5, 0.5)), ball, Sphere((2.5, 0.8, 1.0), 0.8, _mat(0.2, 0.3, 0.9)),
            ball]
    cam = scenes._camera(w, h, (0.0, 4.0, 9.0), (0.0, 1.0, 0.0))
    cfg = RaytracerConfig(max_depth=1, samples_per_pixel=1, width=w, height=h, mode="lambert_shadow", jitter="center")
    sc = LoweredScene(objs, _lights(), cam)
    assert (sc.prims[1].kind, sc.prims[3].kind) == (8, 8)
    assert (sc.prims[1].sdf_first, sc.prims[1].sdf_count) == (sc.prims[3].sdf_first, sc.prims[3].sdf_count)
    assert sc.ir.num_mesh_indices == 3 * ball.num_triangles
    compare(objs, _lights(), cam, cfg)
    ctx = Context(0, jit=abi.JIT_OFF)
    _render(ctx, sc, cfg.lower())
    mi = ctx.mesh_info()
    assert (mi.ranges, mi.bvh_builds, mi.tri_slots) == (1, 1, ball.num_triangles)
    ctx.close()


# ------------------------------------------------------------------------------ 10. multi-GPU
@pytest.mark.parametrize("nranks", [2, 4, 8])
def test_emulated_peers_render_instances_exactly(nranks, monkeypatch):
    import torch
    w, h = 1920, 1080
    objs, lights, cam, cfg = scenes.instance_demo(w, h, detail=DETAIL)
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    plain = np.zeros(w * h * 4, dtype=np.uint8)
    ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), plain.ctypes.data_as(C.POINTER(C.c_uint8))))
    ctx.close()
    assert len(np.unique(plain.reshape(-1, 4), axis=0)) > 100
    monkeypatch.setenv("RRTE_FORCE_GATHER", "1")
    monkeypatch.setenv("RRTE_EMULATE_PEERS", str(nranks))
    ctx = Context(0, jit=abi.JIT_OFF)
    lib = ctx.lib
    uid = (C.c_uint8 * abi.UNIQUE_ID_BYTES)()
    ctx.check(lib.rrte_hip_comm_unique_id(uid))
    ctx.check(lib.rrte_hip_comm_init(ctx.h, 1, 0, uid))
    sky, rb, pb = abi.band_layout(sc.ref(), C.byref(prm), nranks)
    for r in range(1, nranks):
        assert lib.rrte_hip_band_rows_for_rank_ex(h, 16, nranks, r, sky, rb, pb) > 0, r
    out = torch.full((w * h,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(lib.rrte_hip_render_gather_async(ctx.h, sc.ref(), C.byref(prm), 0, out.data_ptr(), None))
    ctx.check(lib.rrte_hip_flush(ctx.h))
    ctx.check(lib.rrte_hip_synchronize(ctx.h))
    got = out.cpu().numpy().view(np.uint8)
    bad = got != plain
    assert not bad.any(), f"N={nranks}: {int(bad.sum())} bytes differ from the plain render"
    ctx.close()


# ------------------------------------------------------------------------ 11. errors and debug
def _status(ctx, sc, prm):
    out = np.empty(prm.width * prm.height * 4, np.uint8)
    return ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_uint8)))


def test_bad_instances_are_refused():
    objs, lights, cam, cfg = thin_scene(16, 9)
    prm = cfg.lower()
    ctx = Context(0, jit=abi.JIT_OFF)

    def fresh():
        return LoweredScene(objs, lights, cam)
    sc = fresh()
    assert sc.prims[1].kind == abi.PRIM_MESH_INSTANCE and _status(ctx, sc, prm) == abi.RRTE_OK
    for slot, value in [(8, 0.0), (7, float("inf")), (9, float("nan")), (0, float("nan")), (1, float("inf")),
                        (4, float("nan"))]:
        sc = fresh()
        sc.prims[1].trs[slot] = value
        assert _status(ctx, sc, prm) == abi.RRTE_INVALID_ARG, (slot, value)
        assert b"instance" in ctx.lib.rrte_hip_last_error(ctx.h)
    sc = fresh()
    sc.prims[1].sdf_count += 1
    assert _status(ctx, sc, prm) == abi.RRTE_INVALID_ARG
    sc = fresh()
    sc.prims[1].sdf_first = sc.ir.num_mesh_indices // 3
    assert _status(ctx, sc, prm) == abi.RRTE_INVALID_ARG
    sc = fresh()
    sc.prims[1].kind = 10
    assert _status(ctx, sc, prm) == abi.RRTE_UNSUPPORTED_PRIM
    # a plain mesh still ignores its trs altogether, zero scale included
    sc = fresh()
    sc.prims[1].kind = abi.PRIM_MESH
    sc.prims[1].trs[7] = 0.0
    assert _status(ctx, sc, prm) == abi.RRTE_OK
    ctx.close()


def test_debug_check_word_stays_clear(monkeypatch):
    monkeypatch.setenv("RRTE_DEBUG", "4")
    objs, lights, cam, cfg = scenes.instance_demo(64, 36, detail=DETAIL)
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    _render(ctx, sc, prm)
    word = C.c_uint64(99)
    ctx.check(ctx.lib.rrte_hip_check_word(ctx.h, C.byref(word)))
    assert word.value == 0
    ctx.close()
