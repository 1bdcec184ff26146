"""Ray queries on the GPU (include/rrte_hip_query.h: rrte_hip_raycast / raycast_async / pick) against a
loop over rrte_oracle_intersect (tests/query_ref.py): objects in list order, strict '<', an SDF object
marched up to min(t_max, best.t) once a hit exists.  prim, front_face and material must be equal and
t, point and normal bit-identical."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import query_ref as q
import scenes_extra as se
from rrte_amd import Color, LambertianMaterial, LoweredScene, Raytracer, Sphere, abi, scenes
from rrte_amd.mesh import icosphere, torus

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
QTOOL = ROOT / "rrte_amd" / "lib" / "cpp_query_tool"

BUILDERS = {name: functools.partial(fn, 64, 36) for name, fn in scenes.SCENES.items()}
for _n in ("mixed_scene", "deformers_scene", "cull_stress_scene", "random_csg_scene"):
    BUILDERS[_n] = functools.partial(getattr(se, _n), 64, 36, "lambert_shadow")
SEGMENT_SCENES = ["mixed_scene", "sdf-showcase", "mesh-demo", "cull_stress_scene"]
TAIL_BUILDERS = {"sdf-showcase": BUILDERS["sdf-showcase"],
                 "mesh-demo": functools.partial(scenes.mesh_demo, 64, 36, detail=0.3)}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def lowered(name):
    objs, lights, cam, _ = scene_of(name)
    return LoweredScene(objs, lights, cam)


def rays_for(segments):
    o, d, length = q.gen_rays()
    return q.rays_of(o, d, q.T_MIN, length if segments else q.INF)


@functools.lru_cache(maxsize=None)
def want_closest(name, segments):
    w = q.oracle_closest(lowered(name), rays_for(segments))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def want_any(name):
    w = q.oracle_any(lowered(name), rays_for(True))
    w.setflags(write=False)
    return w


def raycast(rt, name, segments, any_hit=False):
    objs, lights, _, _ = scene_of(name)
    o, d, length = q.gen_rays()
    return rt.raycast(objs, o, d, t_min=q.T_MIN, t_max=length if segments else q.INF, any_hit=any_hit, lights=lights)


def non_finite(hits):
    hit = hits["prim"] >= 0
    return hit & ~(np.isfinite(hits["t"]) & np.isfinite(hits["point"]).all(1) & np.isfinite(hits["normal"]).all(1))


@pytest.mark.parametrize("name", list(BUILDERS))
def test_closest_hit_matches_the_oracle_loop(name):
    want = want_closest(name, False)
    n = len(want)
    hits = int((want["prim"] >= 0).sum())
    print(name, "oracle: hits", hits, "of", n, "distinct objects", len(set(want["prim"][want["prim"] >= 0])),
          "non-finite", int(non_finite(want).sum()))
    # no scene passes vacuously
    assert n == q.N_RAYS and 2 * hits >= n and 10 * (n - hits) >= n and 100 * int(non_finite(want).sum()) <= n
    got = raycast(Raytracer(scene_of(name)[3], device=0), name, False)
    q.assert_hits_equal(got, want)
    # the records of meshes aside, no triangle index
    kinds = np.array([p.kind for p in lowered(name).prims[:lowered(name).ir.num_prims]])
    on_mesh = (got["prim"] >= 0) & (kinds[np.maximum(got["prim"], 0)] == abi.PRIM_MESH)
    assert not got["tri"][~on_mesh].any()


@pytest.mark.parametrize("name", SEGMENT_SCENES)
def test_finite_segments_closest_and_any(name):
    """t_max = |target - origin| in both query kinds: CLOSEST against the same oracle loop, ANY's prim
    the lowest index whose rrte_oracle_intersect reports a hit."""
    wc, wa = want_closest(name, True), want_any(name)
    occluded = int((wa["prim"] >= 0).sum())
    print(name, "oracle: occluded segments", occluded, "of", len(wa))
    assert occluded >= 10 and len(wa) - occluded >= 10
    assert np.array_equal(wa["prim"] >= 0, wc["prim"] >= 0)  # (the checker itself: occluded = has a closest hit)
    rt = Raytracer(scene_of(name)[3], device=0)
    q.assert_hits_equal(raycast(rt, name, True), wc)
    ga = raycast(rt, name, True, any_hit=True)
    q.assert_hits_equal(ga, wa, tri=True)


@functools.lru_cache(maxsize=None)
def tail_full_run(name):
    objs, lights, _, cfg = TAIL_BUILDERS[name]()
    o, d, _ = q.gen_rays()
    full = Raytracer(cfg, device=0).raycast(objs, o, d, t_min=q.T_MIN, lights=lights)
    full.setflags(write=False)
    return full


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("name", list(TAIL_BUILDERS))
def test_tail_shapes(name, n):
    """n around one wave: the first n of the 517-ray run, and nothing written past n."""
    objs, lights, cam, cfg = TAIL_BUILDERS[name]()
    full = tail_full_run(name)
    assert (full["prim"][:65] >= 0).any() and (full["prim"][:65] < 0).any()
    o, d, _ = q.gen_rays()
    rays = q.rays_of(o[:n], d[:n])
    guard = 64
    hits = np.zeros(n + guard, dtype=abi.RAY_HIT_DTYPE)
    hits.view(np.uint8)[:] = 0xA5
    sentinel = hits.copy()
    rt = Raytracer(cfg, device=0)
    sc = LoweredScene(objs, lights, cam)
    for flags in (abi.QUERY_CLOSEST, abi.QUERY_ANY):
        hits[:] = sentinel
        rt.ctx.check(rt.ctx.lib.rrte_hip_raycast(rt.ctx.h, sc.ref(), rays.ctypes.data_as(C.POINTER(abi.Ray)), n, flags,
                                                 hits.ctypes.data_as(C.POINTER(abi.RayHit))))
        assert hits[n:].tobytes() == sentinel[n:].tobytes()
        if flags == abi.QUERY_CLOSEST:
            assert hits[:n].tobytes() == full[:n].tobytes()
        else:  # every ray runs to +inf: occluded exactly where it has a closest hit
            assert np.array_equal(hits["prim"][:n] >= 0, full["prim"][:n] >= 0)
            assert not hits["t"][:n].any() and not hits["point"][:n].any()


def test_mesh_triangle_index():
    """Two small meshes queried as meshes and as the same triangles lowered one by one: the same hit bit
    for bit, and `tri` names the triangle that wins in the second form."""
    mat = LambertianMaterial(Color.rgb(0.7, 0.5, 0.3))
    meshes = [icosphere((-1.2, 1.0, 0.0), 0.9, 2, mat), torus((1.3, 1.0, 0.0), 0.8, 0.3, 16, 8, mat)]
    ground = Sphere((0, -1000, 0), 1000, LambertianMaterial(Color.rgb(0.3, 0.3, 0.3)))
    as_mesh = [ground] + meshes
    as_tris = [ground] + [t for m in meshes for t in m.triangles()]
    rng = np.random.default_rng(7)
    n = 517
    o = rng.uniform([-4.0, 0.3, -4.0], [4.0, 4.0, 4.0], (n, 3)).astype(np.float32)
    tg = rng.uniform([-2.2, 0.2, -0.9], [2.2, 1.8, 0.9], (n, 3)).astype(np.float32)
    d = (tg - o) * rng.uniform(0.1, 3.0, n).astype(np.float32)[:, None]
    rt = Raytracer(device=0)
    hm = rt.raycast(as_mesh, o, d)
    ht = Raytracer(device=0).raycast(as_tris, o, d)
    for f in ("t", "point", "normal"):
        assert np.array_equal(np.ascontiguousarray(hm[f]).view(np.uint32), np.ascontiguousarray(ht[f]).view(np.uint32)), f
    assert np.array_equal(hm["front_face"], ht["front_face"]) and np.array_equal(hm["material"], ht["material"])
    first = np.cumsum([1] + [m.num_triangles for m in meshes])  # object index of each mesh's first triangle
    on_mesh = hm["prim"] >= 1
    assert on_mesh.sum() >= 100 and len(set(hm["prim"][on_mesh])) == 2
    assert np.array_equal(first[hm["prim"][on_mesh] - 1] + hm["tri"][on_mesh], ht["prim"][on_mesh])
    assert np.array_equal(hm["prim"][~on_mesh], ht["prim"][~on_mesh]) and not hm["tri"][~on_mesh].any()
    # hit_objects: the Python object, and for a mesh the triangle
    who = Raytracer.hit_objects(as_mesh, hm)
    k = int(np.flatnonzero(on_mesh)[0])
    assert who[k] == (meshes[hm["prim"][k] - 1], int(hm["tri"][k]))
    assert all((w is None) == (p < 0) for w, p in zip(who, hm["prim"]))
    assert all(w is ground for w, p in zip(who, hm["prim"]) if p == 0)


PICK_SCENES = {"sdf-showcase": lambda w, h: scenes.sdf_showcase(w, h),
               "ortho_scene": lambda w, h: se.ortho_scene(w, h, "lambert_shadow")}


@pytest.mark.parametrize("w,h", [(33, 19), (1, 1)])
@pytest.mark.parametrize("name", list(PICK_SCENES))
def test_pick_every_pixel(name, w, h):
    objs, lights, cam, cfg = PICK_SCENES[name](w, h)
    ys, xs = np.divmod(np.arange(w * h), w)
    sc = LoweredScene(objs, lights, cam)
    want = q.oracle_closest(sc, q.oracle_pick_rays(sc, w, h, xs, ys, cfg.t_min))
    if w > 1:
        assert 0 < (want["prim"] >= 0).sum() and len(set(want["prim"])) >= 3
    rt = Raytracer(cfg, device=0)
    q.assert_hits_equal(rt.pick(objs, cam, xs, ys, lights=lights), want)
    for bad in ((w, 0), (0, h)):  # a coordinate equal to the width / height
        with pytest.raises(abi.RrteError) as e:
            rt.pick(objs, cam, [0, bad[0]], [0, bad[1]], lights=lights)
        assert e.value.status == abi.RRTE_INVALID_ARG


@pytest.mark.parametrize("jit", [abi.JIT_OFF, abi.JIT_ON])
def test_queries_coexist_with_rendering(jit):
    """render, query, render with one Raytracer: both frames are a fresh context's frame, the
    statistics those of the renders alone, and the query of the cached scene uploads nothing."""
    name = "sdf-showcase"
    objs, lights, cam, cfg = scene_of(name)
    fresh = Raytracer(cfg, device=0, jit=jit)
    want8, wantf = fresh.render_f32(objs, lights, [], cam, linear=True)
    ws = fresh.stats()
    rt = Raytracer(cfg, device=0, jit=jit)
    a8, af = rt.render_f32(objs, lights, [], cam, linear=True)
    s1 = rt.stats()
    got = raycast(rt, name, False)
    s2 = rt.stats()
    ys, xs = np.divmod(np.arange(cfg.width * cfg.height), cfg.width)
    rt.pick(objs, cam, xs, ys, lights=lights)
    b8, bf = rt.render_f32(objs, lights, [], cam, linear=True)
    s3 = rt.stats()
    q.assert_hits_equal(got, want_closest(name, False))
    for g8, gf in ((a8, af), (b8, bf)):
        assert np.array_equal(g8, want8) and np.array_equal(gf.view(np.uint32), wantf.view(np.uint32))
    for s in (s1, s2, s3):
        assert (s.primary_rays, s.shadow_rays) == (ws.primary_rays, ws.shadow_rays)
        assert s.jit_active == (1 if jit == abi.JIT_ON else 0)
    assert (s1.frames, s2.frames, s3.frames) == (1, 1, 2)
    assert s3.upload_ms == 0.0  # the scene stayed cached across the queries


def test_async_form_matches_blocking():
    import torch
    name = "cull_stress_scene"
    objs, lights, _, cfg = scene_of(name)
    rays = rays_for(True)
    n = len(rays)
    rt = Raytracer(cfg, device=0)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    stream = torch.cuda.Stream()
    for any_hit in (False, True):
        d_hits = torch.full((n * 48 + 48,), 0xA5, dtype=torch.uint8, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        rt.raycast_async(objs, d_rays.data_ptr(), n, d_hits.data_ptr(), stream=C.c_void_p(stream.cuda_stream),
                         any_hit=any_hit, lights=lights)
        stream.synchronize()
        out = d_hits.cpu().numpy()
        assert (out[n * 48:] == 0xA5).all()
        got = out[:n * 48].view(abi.RAY_HIT_DTYPE)
        assert got.tobytes() == raycast(rt, name, True, any_hit=any_hit).tobytes()
        q.assert_hits_equal(got, want_any(name) if any_hit else want_closest(name, True), tri=any_hit)
    rt.ctx.check(rt.ctx.lib.rrte_hip_synchronize(rt.ctx.h))
    assert rt.stats().frames == 0


def test_cpp_mirror_raycast_matches_python(tmp_path):
    subprocess.run(["make", "-s", "-C", str(ROOT / "rrte_amd" / "cpp")], check=True)
    objs, lights, cam, cfg = scenes.sdf_showcase(64, 36)
    rays = rays_for(True)
    (tmp_path / "rays.bin").write_bytes(rays.tobytes())
    rt = Raytracer(cfg, device=0)
    for kind in ("closest", "any"):
        out = tmp_path / f"{kind}.bin"
        r = subprocess.run([str(QTOOL), "raycast", "sdf-showcase", str(tmp_path / "rays.bin"), str(out), kind],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"raycast {len(rays)} rays frames 0" in r.stdout
        want = rt.raycast(objs, rays["origin"], rays["direction"], t_min=rays["t_min"], t_max=rays["t_max"],
                          any_hit=kind == "any", lights=lights)
        assert out.read_bytes() == want.tobytes()
    out = tmp_path / "pick.bin"
    r = subprocess.run([str(QTOOL), "pick", "sdf-showcase", "33", "19", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    objs, lights, cam, cfg = scenes.sdf_showcase(33, 19)
    ys, xs = np.divmod(np.arange(33 * 19), 33)
    assert out.read_bytes() == Raytracer(cfg, device=0).pick(objs, cam, xs, ys, lights=lights).tobytes()


def test_error_paths_leave_the_context_usable():
    name = "sdf-showcase"
    objs, lights, cam, cfg = scene_of(name)
    sc = LoweredScene(objs, lights, cam)
    rays = rays_for(False)
    n = len(rays)
    hits = np.zeros(n, dtype=abi.RAY_HIT_DTYPE)
    rt = Raytracer(cfg, device=0)
    lib, h = rt.ctx.lib, rt.ctx.h
    pr, ph = rays.ctypes.data_as(C.POINTER(abi.Ray)), hits.ctypes.data_as(C.POINTER(abi.RayHit))
    prm = cfg.lower()
    xy = np.zeros(2, dtype=np.uint32)
    pxy = xy.ctypes.data_as(C.POINTER(C.c_uint32))
    bad = [lib.rrte_hip_raycast(h, None, pr, n, 0, ph), lib.rrte_hip_raycast(h, sc.ref(), None, n, 0, ph),
           lib.rrte_hip_raycast(h, sc.ref(), pr, n, 0, None), lib.rrte_hip_raycast(h, sc.ref(), pr, 0, 0, ph),
           lib.rrte_hip_raycast(h, sc.ref(), pr, n, 2, ph), lib.rrte_hip_raycast(h, sc.ref(), pr, n, 0x80000001, ph),
           lib.rrte_hip_raycast_async(h, sc.ref(), None, n, 0, None, None),
           lib.rrte_hip_raycast_async(h, sc.ref(), C.c_void_p(16), 0, 0, C.c_void_p(16), None),
           lib.rrte_hip_raycast_async(h, sc.ref(), C.c_void_p(8), n, 0, C.c_void_p(16), None),
           lib.rrte_hip_pick(h, sc.ref(), None, pxy, 1, ph), lib.rrte_hip_pick(h, sc.ref(), C.byref(prm), None, 1, ph),
           lib.rrte_hip_pick(h, sc.ref(), C.byref(prm), pxy, 0, ph),
           lib.rrte_hip_pick(h, None, C.byref(prm), pxy, 1, ph)]
    assert bad == [abi.RRTE_INVALID_ARG] * len(bad)
    assert lib.rrte_hip_last_error(h)
    assert lib.rrte_hip_raycast(None, sc.ref(), pr, n, 0, ph) == abi.RRTE_INVALID_ARG
    # a malformed SDF program: a CSG op with nothing on the value stack
    broken = LoweredScene(objs, lights, cam)
    first = next(p.sdf_first for p in broken.prims if p.kind == abi.PRIM_SDF)
    broken.nodes[first].op = abi.SDF_UNION
    assert lib.rrte_hip_raycast(h, broken.ref(), pr, n, 0, ph) == abi.RRTE_INVALID_ARG
    assert b"malformed SDF program" in lib.rrte_hip_last_error(h)
    assert lib.rrte_hip_pick(h, broken.ref(), C.byref(prm), pxy, 1, ph) == abi.RRTE_INVALID_ARG
    assert not hits.view(np.uint8).any()  # nothing was written
    # the context still answers and renders correctly
    q.assert_hits_equal(raycast(rt, name, False), want_closest(name, False))
    want8, wantf = Raytracer(cfg, device=0).render_f32(objs, lights, [], cam, linear=True)
    got8, gotf = rt.render_f32(objs, lights, [], cam, linear=True)
    assert np.array_equal(got8, want8) and np.array_equal(gotf.view(np.uint32), wantf.view(np.uint32))
    assert rt.stats().frames == 1


def test_call_larger_than_one_staging_chunk():
    """The blocking form stages at most 2^22 rays per launch: a call of 2^22 + 65 rays (a second
    launch whose last wave has one live lane) returns the 517-ray answers, repeated."""
    name = "sdf-showcase"
    objs, lights, _, cfg = scene_of(name)
    o, d, _ = q.gen_rays()
    n = (1 << 22) + 65
    rt = Raytracer(cfg, device=0)
    got = rt.raycast(objs, np.resize(o, (n, 3)), np.resize(d, (n, 3)), t_min=q.T_MIN, lights=lights)
    small = rt.raycast(objs, o, d, t_min=q.T_MIN, lights=lights)
    q.assert_hits_equal(small, want_closest(name, False))
    assert got.tobytes() == np.resize(small, n).tobytes()
