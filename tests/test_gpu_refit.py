"""Deforming meshes on the device (include/rrte_hip_refit.h): after rrte_hip_mesh_refit
the next scene version's BVHs are refitted by the refit kernels instead of rebuilt on the host.

A mesh is the closest hit over its triangles in index order, so a refitted tree must report bit for
bit what the oracle's linear scan reports for a fresh lowering of the deformed meshes: frames (generic,
full-JIT and topology kernels), ray queries, instances of a deformed base, frames in flight, emulated
peers.  The boxes themselves are compared bit for bit with tests/refit_ref.py through
rrte_hip_mesh_nodes, and a refit of unchanged vertices must reproduce the built records exactly.

The meshes: icosphere(2) (320 triangles), heightfield(9) (128), a 4-triangle fan (its root is a leaf:
no record) and a single triangle; one coordinate is -0.0.  The deformation twists, adds a sine of an
amplitude comparable to the mesh and translates by more than the mesh's diameter, so stale boxes
would miss everything.  Leaves of more than 4 triangles arise only at depth 31: no mesh of this size
reaches them (refit_ref's synthetic tree covers the count field on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import instance_ref as ir
import oracle
import query_ref as q
import refit_ref as rr
from rrte_amd import (Camera, Color, LambertianMaterial, LoweredScene, MeshInstance, PointLight, Raytracer,
                      RaytracerConfig, Sphere, Transform, abi, scenes)
from rrte_amd.mesh import Mesh, heightfield, icosphere
from rrte_amd.renderer import Context

# (the single-triangle mesh has a vertex nothing names: its recomputed normal is 0 / 0, and unused)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]

F = np.float32
SHIFT = np.array([7.0, 0.5, 5.0])  # |SHIFT| = 8.6: more than the diagonal of any of the meshes' boxes (<= 7.7)


def _mat(r, g, b):
    return LambertianMaterial(Color.rgb(r, g, b))


def _lights():
    return [PointLight((-10.0, 15.0, 10.0), Color.rgb(1.0, 1.0, 1.0), 25.0),
            PointLight((10.0, 10.0, 15.0), Color.rgb(0.6, 0.7, 1.0), 15.0)]


def deform(base, k):
    """Pose k of (N, 3) positions: pose 0 is `base`; pose k > 0 twists about the vertical through the
    centroid, displaces by a sine of amplitude ~ a third of the mesh and translates by SHIFT (+ a
    little per pose), in float64, rounded once."""
    if k == 0:
        return base.copy()
    p = base.astype(np.float64)
    c = p.mean(0)
    qv = p - c
    size = max(np.ptp(p, axis=0).max(), 1e-3)
    ang = (0.9 + 0.2 * k) * qv[:, 1] / size * 2.0 + 0.4 * k
    x = qv[:, 0] * np.cos(ang) - qv[:, 2] * np.sin(ang)
    z = qv[:, 0] * np.sin(ang) + qv[:, 2] * np.cos(ang)
    y = qv[:, 1] + 0.3 * size * np.sin(4.0 * x / size + k)
    return (np.stack([x, y, z], 1) + c + SHIFT + 0.15 * (k - 1)).astype(F)


class Rig:
    """Ground, the four meshes, a small sphere; set_pose(k) deforms every mesh in place."""

    def __init__(self):
        ball = icosphere((-4.0, 2.3, -3.0), 2.2, 2, _mat(0.8, 0.3, 0.3))
        field = heightfield((-7.0, 0.4, 0.0), 5.0, 9, lambda x, z: 0.5 * np.sin(x) * np.cos(z), _mat(0.3, 0.7, 0.4))
        fan = Mesh(np.array([[-1.0, 1.5, -6.0], [-3.0, 0.2, -7.5], [1.0, 0.2, -7.5], [1.0, 2.8, -4.5], [-3.0, 2.8, -4.5]], F),
                   np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], np.uint32), None, _mat(0.2, 0.4, 0.9))
        # one triangle and a vertex nothing names (test_argument_errors makes it non-finite)
        tri = Mesh(np.array([[-2.0, 0.3, 5.0], [0.5, 0.3, 5.5], [-1.0, 3.0, 5.0], [0.0, 9.0, 0.0]], F),
                   np.array([[0, 1, 2]], np.uint32), None, _mat(0.9, 0.8, 0.2))
        self.meshes = [ball, field, fan, tri]
        assert [m.num_triangles for m in self.meshes] == [320, 128, 4, 1]
        self.base = [m.positions.copy() for m in self.meshes]
        assert all(np.linalg.norm(np.ptp(b[:3] if i == 3 else b, axis=0)) < np.linalg.norm(SHIFT)
                   for i, b in enumerate(self.base))
        self.ground = Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.5, 0.5, 0.5))
        self.marble = Sphere((3.0, 0.7, -2.0), 0.7, _mat(0.9, 0.9, 0.9))
        self.lights = _lights()

    def set_pose(self, k):
        for m, b in zip(self.meshes, self.base):
            p = deform(b, k)
            if m.num_triangles == 4 and k:
                p[2, 0] = F(-0.0)  # a negative zero among the coordinates
            m.set_vertices(p)
        return self

    def objects(self):
        return [self.ground, *self.meshes, self.marble]

    def scene(self, w=64, h=36, lights=True):
        return LoweredScene(self.objects(), self.lights if lights else [], cam(w, h))


def cam(w, h):
    return scenes._camera(w, h, (1.0, 7.0, 16.0), (1.0, 1.5, 0.0))


def cfg_of(w, h, mode="lambert_shadow"):
    return RaytracerConfig(max_depth=1, samples_per_pixel=1, width=w, height=h, mode=mode, jitter="center")


def _render(ctx, sc, prm, linear=True):
    p = abi.RenderParams.from_buffer_copy(prm)
    if linear:
        p.flags |= abi.FLAG_F32_LINEAR
    n = p.width * p.height * 4
    out8, outf = np.empty(n, np.uint8), np.empty(n, np.float32)
    ctx.check(ctx.lib.rrte_hip_render_f32(ctx.h, sc.ref(), C.byref(p), out8.ctypes.data, outf.ctypes.data))
    return out8, outf, ctx.stats()


def _touch(ctx, sc):
    """Makes `sc` the context's scene (upload, BVH build) without a frame: one ray query."""
    rays = q.rays_of(np.zeros((1, 3), F), np.array([[0.0, -1.0, 0.0]], F))
    hits = np.zeros(1, dtype=abi.RAY_HIT_DTYPE)
    ctx.check(ctx.lib.rrte_hip_raycast(ctx.h, sc.ref(), rays.ctypes.data_as(C.POINTER(abi.Ray)), 1, abi.QUERY_CLOSEST,
                                       hits.ctypes.data_as(C.POINTER(abi.RayHit))))


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


def _check_frame(ctx, sc, prm, want, expect_jit=None):
    r8, lin, shadow = want
    g8l, glin, st = _render(ctx, sc, prm)
    if expect_jit is not None:
        assert st.jit_active == expect_jit
    bad = np.flatnonzero(glin.view(np.uint32) != lin.view(np.uint32))
    assert bad.size == 0, (bad.size, bad[:8] // 4, glin[bad[:8]], lin[bad[:8]])
    assert int(st.shadow_rays) == shadow
    g8, _, _ = _render(ctx, sc, prm, linear=False)
    assert np.abs(g8.astype(np.int16) - r8.astype(np.int16)).max() <= 1
    return g8, glin


def _covers(want, ground_only):
    """Pixels where the frame differs from the frame of the ground alone."""
    return int((want[1].view(np.uint32).reshape(-1, 4) != ground_only[1].view(np.uint32).reshape(-1, 4)).any(1).sum())


# ------------------------------------------------------------------------------- 1. identity
def test_refit_of_unchanged_vertices_reproduces_the_build():
    rig = Rig().set_pose(1)
    prm = cfg_of(64, 36).lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    sc = rig.scene()
    _, lin_a, _ = _render(ctx, sc, prm)
    nodes_a = ctx.mesh_nodes()
    mi, ri = ctx.mesh_info(), ctx.refit_info()
    assert (mi.ranges, mi.bvh_builds, mi.tri_slots) == (4, 4, 453) and mi.bvh_nodes == len(nodes_a) > 100
    assert (ri.refits, ri.device_refits, ri.levels, ri.deformed) == (0, 0, 0, 0)
    # the same vertices in new arrays under a new version
    sc2 = rig.scene()
    assert sc2.ir.mesh_version != sc.ir.mesh_version and sc2._mesh_vtx.ctypes.data != sc._mesh_vtx.ctypes.data
    assert np.array_equal(sc2._mesh_vtx.view(np.uint32), sc._mesh_vtx.view(np.uint32))
    ctx.mesh_refit(sc2)
    ri = ctx.refit_info()
    assert (ri.refits, ri.device_refits, ri.deformed) == (1, 0, 1) and ri.levels >= 5
    _, lin_b, _ = _render(ctx, sc2, prm)
    nodes_b = ctx.mesh_nodes()
    assert nodes_a.shape == nodes_b.shape and np.array_equal(nodes_a.view(np.uint32), nodes_b.view(np.uint32))
    assert np.array_equal(lin_a.view(np.uint32), lin_b.view(np.uint32))
    ri2 = ctx.refit_info()
    assert (ri2.refits, ri2.device_refits, ri2.levels, ri2.deformed) == (1, 1, ri.levels, 1)
    assert ctx.mesh_info().bvh_builds == 4
    # levels = the deepest record's depth: launches of refit_level per refit
    links = rr.links_of(nodes_a)
    depth = {r: 0 for r in rr.roots_of(nodes_a)}
    todo = list(depth)
    while todo:
        r = todo.pop()
        for link in links[r]:
            if not int(link) & rr.LEAF_BIT:
                depth[int(link)] = depth[r] + 1
                todo.append(int(link))
    assert len(depth) == len(nodes_a) and ri.levels == max(depth.values())
    ctx.close()


# ---------------------------------------------------------------------------------- 2. boxes
def test_refitted_boxes_equal_the_checker_bit_for_bit():
    rig = Rig()
    prm = cfg_of(64, 36).lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    sc0 = rig.scene()
    _touch(ctx, sc0)
    built = ctx.mesh_nodes()
    slot_vtx = rr.slot_vertex_table(sc0, ctx.mesh_slots())
    # the build itself is what the checker computes from pose 0
    same, _ = rr.refit(built, slot_vtx, sc0._mesh_vtx[:, :3])
    assert np.array_equal(same.view(np.uint32), built.view(np.uint32))
    for k in (1, 2):
        sc = rig.set_pose(k).scene()
        ctx.mesh_refit(sc)
        _render(ctx, sc, prm)
        got = ctx.mesh_nodes()
        want, tops = rr.refit(built, slot_vtx, sc._mesh_vtx[:, :3])
        assert np.array_equal(got.view(np.uint32)[:, :, 3], built.view(np.uint32)[:, :, 3])  # links and axes kept
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=(1, 2)))
        assert bad.size == 0, (k, bad[:8], got[bad[:2]], want[bad[:2]])
        assert (got.view(np.uint32) != built.view(np.uint32)).any(axis=(1, 2)).all()  # every record moved
        assert np.array_equal(rr.slot_vertex_table(sc, ctx.mesh_slots()), slot_vtx)  # the slots stay put
    assert ctx.refit_info().device_refits == 2 and ctx.mesh_info().bvh_builds == 4
    ctx.close()


# --------------------------------------------------------------------------------- 3. frames
VARIANTS = {"generic": (abi.JIT_OFF, None, 0), "full": (abi.JIT_ON, "0", 1), "topology": (abi.JIT_ON, "1", 2)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
@pytest.mark.parametrize("w,h", [(64, 36), (67, 37)])
def test_refitted_frames_match_the_oracle(w, h, mode, variant, monkeypatch):
    jit, topo, expect = VARIANTS[variant]
    if topo is None:
        monkeypatch.delenv("RRTE_JIT_TOPO", raising=False)
    else:
        monkeypatch.setenv("RRTE_JIT_TOPO", topo)
    rig = Rig()
    prm = cfg_of(w, h, mode).lower()
    sc0 = rig.scene(w, h)
    sc1 = rig.set_pose(1).scene(w, h)
    want = _oracle_frame(("pose1", w, h, mode), sc1, prm)
    ground = _oracle_frame(("ground", w, h, mode), LoweredScene([rig.ground, rig.marble], rig.lights, cam(w, h)), prm)
    assert _covers(want, ground) > w * h // 12, "the deformed meshes hardly show"
    frames = []
    for tile_cull in ("1", "0"):  # 0: no camera-ray tile culling, so the culling spheres cannot matter
        monkeypatch.setenv("RRTE_TILE_CULL", tile_cull)
        ctx = Context(0, jit=jit)
        _touch(ctx, sc0)
        ctx.mesh_refit(sc1)
        frames.append(_check_frame(ctx, sc1, prm, want, expect))
        ri = ctx.refit_info()
        assert (ri.refits, ri.device_refits, ri.deformed) == (1, 1, 1) and ctx.mesh_info().bvh_builds == 4
        ctx.close()
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1].view(np.uint32), frames[1][1].view(np.uint32))


# -------------------------------------------------------------------------------- 4. queries
def _query_rays():
    o, d, length = q.gen_rays()
    assert len(o) == 517
    t_max = np.where(np.arange(len(o)) % 3 == 0, length * np.float32(0.8), q.INF).astype(np.float32)
    return q.rays_of(o, d, q.T_MIN, t_max)


def _raycast(ctx, sc, rays, any_hit):
    hits = np.zeros(len(rays), dtype=abi.RAY_HIT_DTYPE)
    ctx.check(ctx.lib.rrte_hip_raycast(ctx.h, sc.ref(), rays.ctypes.data_as(C.POINTER(abi.Ray)), len(rays),
                                       abi.QUERY_ANY if any_hit else abi.QUERY_CLOSEST,
                                       hits.ctypes.data_as(C.POINTER(abi.RayHit))))
    return hits


@pytest.mark.parametrize("any_hit", [False, True])
def test_queries_on_refitted_meshes_match_the_checker(any_hit):
    rig = Rig()
    objs = rig.meshes + [rig.marble]  # (no ground: in list order it would occlude every ANY query first)
    sc0 = LoweredScene(objs, [], Camera())
    rig.set_pose(1)
    sc1 = LoweredScene(objs, [], Camera())
    rays = _query_rays()
    want = ir.any_hit(sc1, rays) if any_hit else ir.closest(sc1, rays)
    on_mesh = sum(sc1.prims[i].kind == abi.PRIM_MESH for i in want["prim"][want["prim"] >= 0])
    assert on_mesh > 40, "the rays hardly touch the deformed meshes"
    ctx = Context(0)
    _touch(ctx, sc0)
    ctx.mesh_refit(sc1)
    got = _raycast(ctx, sc1, rays, any_hit)
    q.assert_hits_equal(got, want, tri=True)
    ri = ctx.refit_info()
    assert (ri.device_refits, ri.deformed) == (1, 1) and ctx.mesh_info().bvh_builds == 4
    ctx.close()


# ------------------------------------------------------------------------------ 5. instances
def _family(ball, w, h):
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, _mat(0.5, 0.5, 0.5)), ball,
            MeshInstance(ball, Transform((-9.0, 0.0, -3.0), scenes.Q_Y45, (0.8, 1.1, 0.9)), _mat(0.3, 0.7, 0.4)),
            MeshInstance(ball, Transform((6.0, 0.2, -4.0), scenes.Q_X45, (-0.9, 0.7, 0.8)))]
    return objs


@pytest.mark.parametrize("variant", ["generic", "topology"])
@pytest.mark.parametrize("w,h", [(64, 36), (67, 37)])
def test_instances_of_a_deformed_base(w, h, variant, monkeypatch):
    jit, topo, expect = VARIANTS[variant]
    monkeypatch.setenv("RRTE_JIT_TOPO", topo or "0")
    ball = icosphere((-4.0, 2.3, -3.0), 2.2, 2, _mat(0.8, 0.3, 0.3))
    base = ball.positions.copy()
    objs, lights = _family(ball, w, h), _lights()
    prm = cfg_of(w, h).lower()
    sc0 = LoweredScene(objs, lights, cam(w, h))
    ball.set_vertices(deform(base, 1))
    sc1 = LoweredScene(objs, lights, cam(w, h))
    assert [sc1.prims[i].kind for i in range(4)] == [0, 8, 9, 9] and sc1.prims[3].trs[7] < 0
    want = _oracle_frame(("family", w, h), sc1, prm, lambda s, p, lin: ir.render(monkeypatch, s, p, linear=lin))
    ctx = Context(0, jit=jit)
    _touch(ctx, sc0)
    ctx.mesh_refit(sc1)
    _check_frame(ctx, sc1, prm, want, expect)
    mi = ctx.mesh_info()
    assert (mi.ranges, mi.bvh_builds, mi.tri_slots) == (1, 1, 320) and ctx.refit_info().device_refits == 1
    if variant == "generic" and (w, h) == (64, 36):  # queries: every field, both kinds
        rays = _query_rays()
        for any_hit in (False, True):
            qs = LoweredScene(objs[1:], [], Camera())
            wantq = ir.any_hit(qs, rays) if any_hit else ir.closest(qs, rays)
            kinds = [qs.prims[i].kind for i in wantq["prim"][wantq["prim"] >= 0]]
            assert kinds.count(abi.PRIM_MESH_INSTANCE) >= 10 and len(kinds) > 40
            ctx.mesh_refit(qs)
            q.assert_hits_equal(_raycast(ctx, qs, rays, any_hit), wantq, tri=True)
        assert ctx.mesh_info().bvh_builds == 1 and ctx.mesh_info().ranges == 1
    ctx.close()


# ------------------------------------------------------------------- 6. the stale-cache trap
def test_three_refits_a_moved_sphere_then_an_index_change():
    w, h = 64, 36
    rig = Rig()
    prm = cfg_of(w, h).lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    sc = rig.scene()
    _check_frame(ctx, sc, prm, _oracle_frame(("pose0", w, h, "lambert_shadow"), sc, prm))
    for k in (1, 2, 3):
        sc = rig.set_pose(k).scene()
        ctx.mesh_refit(sc)
        _check_frame(ctx, sc, prm, _oracle_frame((f"pose{k}", w, h, "lambert_shadow"), sc, prm))
        ri = ctx.refit_info()
        assert (ri.refits, ri.device_refits, ri.deformed) == (k, k, 1)
    # only a sphere moves: the same mesh arrays, so the deformed cache is hit and must be refitted
    # again (its host copy is pose 0's)
    assert sc.prims[5].kind == abi.PRIM_SPHERE
    sc.prims[5].p[0], sc.prims[5].p[1], sc.prims[5].p[2] = -2.0, 0.7, 8.0
    _check_frame(ctx, sc, prm, _oracle_frame(("trap-sphere", w, h), sc, prm))
    ri = ctx.refit_info()
    assert (ri.refits, ri.device_refits, ri.deformed) == (3, 4, 1) and ctx.mesh_info().bvh_builds == 4
    # an index change (the fan's first triangle turned over): not a deformation
    fan = rig.meshes[2]
    turned = fan.indices.copy()
    turned[0] = turned[0][::-1]
    rig.meshes[2] = Mesh(fan.positions, turned, None, fan.material)
    sc = rig.scene()
    with pytest.raises(abi.RrteError) as e:
        ctx.mesh_refit(sc)
    assert e.value.status == abi.RRTE_INVALID_ARG and "index" in str(e.value)
    ri = ctx.refit_info()
    assert (ri.refits, ri.device_refits, ri.deformed) == (3, 4, 1)  # refused: as it was
    _check_frame(ctx, sc, prm, _oracle_frame(("trap-index", w, h), sc, prm))
    ri = ctx.refit_info()
    assert (ri.refits, ri.device_refits, ri.deformed) == (3, 4, 0) and ctx.mesh_info().bvh_builds == 8
    ctx.close()


# --------------------------------------------------------------------- 7. frames in flight
def test_a_frame_in_flight_keeps_its_own_pose():
    import torch
    w, h = 64, 36
    rig = Rig().set_pose(1)
    prm = cfg_of(w, h).lower()
    sc_a = rig.scene()
    sc_b = rig.set_pose(2).scene()
    want_a = _oracle_frame(("pose1", w, h, "lambert_shadow"), sc_a, prm)
    want_b = _oracle_frame(("pose2", w, h, "lambert_shadow"), sc_b, prm)
    plain = []
    for sc in (sc_a, sc_b):  # each pose built and rendered on its own context
        c = Context(0, jit=abi.JIT_OFF)
        plain.append(_render(c, sc, prm, linear=False)[0])
        c.close()
    assert not np.array_equal(plain[0], plain[1])
    ctx = Context(0, jit=abi.JIT_OFF)
    buf = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rrte_hip_render_async(ctx.h, sc_a.ref(), C.byref(prm), buf.data_ptr(), None, None))
    ctx.mesh_refit(sc_b)
    got_b = _render(ctx, sc_b, prm, linear=False)[0]
    ctx.check(ctx.lib.rrte_hip_synchronize(ctx.h))
    got_a = buf.cpu().numpy().view(np.uint8)
    assert np.array_equal(got_a, plain[0]) and np.array_equal(got_b, plain[1])
    assert np.abs(got_a.astype(np.int16) - want_a[0].astype(np.int16)).max() <= 1
    assert np.abs(got_b.astype(np.int16) - want_b[0].astype(np.int16)).max() <= 1
    assert ctx.refit_info().device_refits == 1 and ctx.mesh_info().bvh_builds == 4
    ctx.close()


# ----------------------------------------------------------------------- 8. argument errors
def _refused(ctx, sc, word):
    st = ctx.lib.rrte_hip_mesh_refit(ctx.h, sc.ref())
    msg = ctx.lib.rrte_hip_last_error(ctx.h).decode()
    assert st == abi.RRTE_INVALID_ARG and "mesh refit" in msg and word in msg, (st, msg)


@pytest.mark.parametrize("case", ["no cache", "vertex count", "index count", "ranges", "non-finite"])
def test_argument_errors(case):
    w, h = 64, 36
    rig = Rig()
    prm = cfg_of(w, h).lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    if case != "no cache":
        _touch(ctx, rig.scene())
    before = (ctx.mesh_info().bvh_builds, ctx.refit_info().refits)
    rig.set_pose(1)
    tri = rig.meshes[3]
    if case == "no cache":
        sc = rig.scene()
        _refused(ctx, sc, "nothing built")
    elif case == "vertex count":  # one more vertex that nothing names: same indices
        rig.meshes[3] = Mesh(np.vstack([tri.positions, [[1.0, 1.0, 1.0]]]).astype(F), tri.indices, None, tri.material)
        sc = rig.scene()
        _refused(ctx, sc, "vertex count")
    elif case == "index count":  # the fan loses a triangle
        fan = rig.meshes[2]
        rig.meshes[2] = Mesh(fan.positions, fan.indices[:3], None, fan.material)
        sc = rig.scene()
        _refused(ctx, sc, "index count")
    elif case == "ranges":  # the same arrays, but the field's object names one triangle less
        sc = rig.scene()
        assert sc.prims[2].kind == abi.PRIM_MESH and sc.prims[2].sdf_count == 128
        sc.prims[2].sdf_count = 127
        _refused(ctx, sc, "ranges")
    else:  # the vertex nothing names: the scene itself stays well defined
        p = tri.positions.copy()
        p[3, 1] = np.inf
        tri.set_vertices(p, normals=tri.normals)
        sc = rig.scene()
        _refused(ctx, sc, "non-finite")
    ri = ctx.refit_info()
    assert (ctx.mesh_info().bvh_builds, ri.refits, ri.device_refits, ri.deformed) == (*before, 0, 0)
    # the plain render of the new scene simply builds
    _check_frame(ctx, sc, prm, _oracle_frame(("error", case), sc, prm))
    ri = ctx.refit_info()
    assert (ri.refits, ri.device_refits, ri.deformed) == (0, 0, 0) and ctx.mesh_info().bvh_builds == before[0] + 4
    ctx.close()


def test_render_deformed_refits_and_falls_back():
    w, h = 64, 36
    rig = Rig()
    rt = Raytracer(cfg_of(w, h), device=0, jit=abi.JIT_OFF)
    cam_ = cam(w, h)
    first = rt.render_deformed(rig.objects(), rig.lights, [], cam_)  # nothing built yet: refused, builds
    assert (rt.ctx.refit_info().refits, rt.ctx.mesh_info().bvh_builds) == (0, 4)
    assert np.array_equal(first, Raytracer(cfg_of(w, h), device=0, jit=abi.JIT_OFF).render(rig.objects(), rig.lights, [], cam_))
    rig.set_pose(1)
    got8, glin = rt.render_f32_deformed(rig.objects(), rig.lights, [], cam_, linear=True)
    ri = rt.ctx.refit_info()
    assert (ri.refits, ri.device_refits, ri.deformed, rt.ctx.mesh_info().bvh_builds) == (1, 1, 1, 4)
    want = _oracle_frame(("pose1", w, h, "lambert_shadow"), rig.scene(), cfg_of(w, h).lower())
    assert np.array_equal(glin.view(np.uint32), want[1].view(np.uint32))
    again = rt.render_deformed(rig.objects(), rig.lights, [], cam_)
    assert np.abs(again.astype(np.int16) - want[0].astype(np.int16)).max() <= 1
    assert rt.ctx.refit_info().refits == 2
    # the existing methods keep building
    rig.set_pose(2)
    rt.render(rig.objects(), rig.lights, [], cam_)
    assert (rt.ctx.refit_info().deformed, rt.ctx.mesh_info().bvh_builds) == (0, 8)


# -------------------------------------------------------------------- 9. peers and the check word
def test_emulated_peers_render_a_refitted_scene_exactly(monkeypatch):
    import torch
    w, h, nranks = 320, 180, 2
    rig = Rig()
    prm = cfg_of(w, h).lower()
    sc0 = rig.scene(w, h)
    sc1 = rig.set_pose(1).scene(w, h)
    ctx = Context(0, jit=abi.JIT_OFF)
    plain = np.zeros(w * h * 4, dtype=np.uint8)
    ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc1.ref(), C.byref(prm), plain.ctypes.data_as(C.POINTER(C.c_uint8))))
    ctx.close()
    assert len(np.unique(plain.reshape(-1, 4), axis=0)) > 100
    monkeypatch.setenv("RRTE_FORCE_GATHER", "1")
    monkeypatch.setenv("RRTE_EMULATE_PEERS", str(nranks))
    ctx = Context(0, jit=abi.JIT_OFF)
    lib = ctx.lib
    uid = (C.c_uint8 * abi.UNIQUE_ID_BYTES)()
    ctx.check(lib.rrte_hip_comm_unique_id(uid))
    ctx.check(lib.rrte_hip_comm_init(ctx.h, 1, 0, uid))
    sky, rb, pb = abi.band_layout(sc1.ref(), C.byref(prm), nranks)
    assert lib.rrte_hip_band_rows_for_rank_ex(h, 16, nranks, 1, sky, rb, pb) > 0
    _touch(ctx, sc0)
    ctx.mesh_refit(sc1)
    out = torch.full((w * h,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(lib.rrte_hip_render_gather_async(ctx.h, sc1.ref(), C.byref(prm), 0, out.data_ptr(), None))
    ctx.check(lib.rrte_hip_flush(ctx.h))
    ctx.check(lib.rrte_hip_synchronize(ctx.h))
    got = out.cpu().numpy().view(np.uint8)
    bad = got != plain
    assert not bad.any(), f"{int(bad.sum())} bytes differ from the plain render"
    assert ctx.refit_info().device_refits == 1 and ctx.mesh_info().bvh_builds == 4
    ctx.close()


def test_debug_check_word_stays_clear_after_a_refit(monkeypatch):
    monkeypatch.setenv("RRTE_DEBUG", "4")
    rig = Rig()
    prm = cfg_of(64, 36).lower()
    ctx = Context(0, jit=abi.JIT_OFF)
    _touch(ctx, rig.scene())
    sc = rig.set_pose(1).scene()
    ctx.mesh_refit(sc)
    _check_frame(ctx, sc, prm, _oracle_frame(("pose1", 64, 36, "lambert_shadow"), sc, prm))
    assert ctx.refit_info().device_refits == 1
    word = C.c_uint64(99)
    ctx.check(ctx.lib.rrte_hip_check_word(ctx.h, C.byref(word)))
    assert word.value == 0
    ctx.close()
