"""Mesh BVHs built on the device (include/rrte_hip_build.h): under policy DEVICE a
mesh-cache miss runs the LBVH kernels instead of the host's SAH builder.

A mesh is the closest hit over its triangles in index order, ties to the lower index, so a device-built
tree must report bit for bit what the oracle's linear scan reports: frames (generic, full-JIT and
topology kernels), ray queries, refits of a device-built tree, instances, frames in flight, emulated
peers.  The tree itself is compared with tests/lbvh_ref.py (links, axes, slot order, depth) and its
boxes with tests/refit_ref.py, bit for bit, through rrte_hip_mesh_nodes / rrte_hip_mesh_slots.

The meshes, the smallest that reach each branch: icosphere(2) (320 triangles), heightfield(9) (128), a
4-triangle fan (its root is a leaf: no record), a single triangle, 5 triangles (one record, a second
leaf of one triangle), one triangle 9 times over (all codes equal, every hit a tie), and the
caterpillar: 4 triangles in each Morton cell 2^k, two in the far corner, and a cluster in cell 0 that
decides whether the tree fits the traversal stack."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import instance_ref as ir
import lbvh_ref as lr
import query_ref as q
import refit_ref as rr
from rrte_amd import Camera, LoweredScene, Raytracer, abi
from rrte_amd.mesh import Mesh, icosphere
from rrte_amd.renderer import Context
from test_gpu_refit import (VARIANTS, Rig, _check_frame, _covers, _family, _lights, _mat, _oracle_frame, _query_rays,
                            _raycast, _render, _touch, cam, cfg_of, deform)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]

ROOT = Path(__file__).resolve().parents[1]
TOOL = ROOT / "rrte_amd" / "lib" / "cpp_build_tool"
F = np.float32
HOST, DEVICE = abi.MESH_BUILD_HOST, abi.MESH_BUILD_DEVICE


class BuildRig(Rig):
    """Rig's four meshes, a 5-triangle strip and a triangle repeated 9 times."""

    def __init__(self):
        super().__init__()
        strip = Mesh(np.array([[4.0, 0.3, 1.0], [5.2, 0.3, 1.4], [4.1, 1.5, 1.0], [5.3, 1.6, 1.5], [4.2, 2.7, 1.1],
                               [5.4, 2.8, 1.6], [4.3, 3.9, 1.2]], F),
                     np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4], [4, 5, 6]], np.uint32), None, _mat(0.7, 0.2, 0.8))
        nine = Mesh(np.array([[6.0, 0.4, -1.0], [8.5, 0.5, -0.5], [7.0, 3.2, -1.5]], F),
                    np.array([[0, 1, 2]] * 9, np.uint32), None, _mat(0.2, 0.8, 0.8))
        self.meshes += [strip, nine]
        self.base += [strip.positions.copy(), nine.positions.copy()]
        assert [m.num_triangles for m in self.meshes] == [320, 128, 4, 1, 5, 9]


N_RANGES, N_SLOTS = 6, 467


def _device_ctx(jit=abi.JIT_OFF):
    ctx = Context(0, jit=jit)
    ctx.set_mesh_build(DEVICE)
    return ctx


def _counts(ctx):
    bi, mi = ctx.build_info(), ctx.mesh_info()
    return bi.device_builds, bi.host_fallbacks, mi.bvh_builds


def _assert_tree_is_the_reference(ctx, sc):
    """Links, axes, slot order and depth against lbvh_ref; boxes against refit_ref; the slot partition."""
    nodes, slots = ctx.mesh_nodes(), ctx.mesh_slots()
    ref = lr.build_scene(sc)
    u = nodes.view(np.uint32)
    assert np.array_equal(slots, ref["slots"])
    assert u.shape[0] == len(ref["links"]) and np.array_equal(u[:, (0, 2), 3], ref["links"])
    assert np.array_equal(u[:, 1, 3], ref["axis"]) and (u[:, 1, 3] <= 2).all() and (u[:, 3, 3] == 0).all()
    slot_vtx = rr.slot_vertex_table(sc, slots)
    want, _ = rr.refit(nodes, slot_vtx, sc._mesh_vtx[:, :3])
    bad = np.flatnonzero((want.view(np.uint32) != u).any(axis=(1, 2)))
    assert bad.size == 0, (bad[:8], nodes[bad[:2]], want[bad[:2]])
    base, covered = 0, np.zeros(len(slots), np.int64)
    for (first, count), r in zip(lr.scene_ranges(sc), ref["ranges"]):
        assert sorted(slots[base:base + count].tolist()) == list(range(count))  # every triangle in exactly one slot
        leaf_links = [r["root"]] if r["root"] & lr.LEAF_BIT and count else [int(x) for x in r["links"].reshape(-1) if x & lr.LEAF_BIT]
        for link in leaf_links:
            a, n = rr.leaf_slots(link)
            assert 1 <= n <= 4 and base <= a and a + n <= base + count
            covered[a:a + n] += 1
        base += count
    assert (covered == 1).all()
    assert ctx.build_info().depth == ref["depth"]
    return ref


# ------------------------------------------------------------------------------ 1. structure
def test_structure_is_the_reference_tree():
    rig = BuildRig()
    sc = rig.scene()
    ctx = _device_ctx()
    assert _counts(ctx) == (0, 0, 0) and ctx.build_info().depth == 0 and ctx.build_info().policy == DEVICE
    _touch(ctx, sc)
    ref = _assert_tree_is_the_reference(ctx, sc)
    assert [len(r["links"]) for r in ref["ranges"]] == [79, 31, 0, 0, 1, 2] and ref["depth"] >= 7
    mi = ctx.mesh_info()
    assert _counts(ctx) == (N_RANGES, 0, N_RANGES) and (mi.ranges, mi.tri_slots, mi.bvh_nodes) == (N_RANGES, N_SLOTS, 113)
    assert ref["ranges"][5]["order"].tolist() == list(range(9))  # equal codes: index order
    assert ref["ranges"][0]["order"].tolist() != list(range(320))  # the sort moved something
    ctx.close()


# --------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
@pytest.mark.parametrize("w,h", [(64, 36), (67, 37)])
def test_frames_on_device_built_trees_match_the_oracle(w, h, mode, variant, monkeypatch):
    jit, topo, expect = VARIANTS[variant]
    if topo is None:
        monkeypatch.delenv("RRTE_JIT_TOPO", raising=False)
    else:
        monkeypatch.setenv("RRTE_JIT_TOPO", topo)
    rig = BuildRig()
    prm = cfg_of(w, h, mode).lower()
    sc = rig.scene(w, h)
    want = _oracle_frame(("build", w, h, mode), sc, prm)
    ground = _oracle_frame(("ground0", w, h, mode), LoweredScene([rig.ground, rig.marble], rig.lights, cam(w, h)), prm)
    assert _covers(want, ground) > w * h // 12, "the meshes hardly show"
    frames = []
    for tile_cull in ("1", "0"):  # 0: no camera-ray tile culling, so the culling spheres cannot matter
        monkeypatch.setenv("RRTE_TILE_CULL", tile_cull)
        ctx = _device_ctx(jit)
        frames.append(_check_frame(ctx, sc, prm, want, expect))
        assert _counts(ctx) == (N_RANGES, 0, N_RANGES)
        # the same context back on the host builder: new arrays under a new version, the same frame
        ctx.set_mesh_build(HOST)
        sc2 = rig.scene(w, h)
        assert sc2.ir.mesh_version != sc.ir.mesh_version
        _, lin_host, st = _render(ctx, sc2, prm)
        assert np.array_equal(lin_host.view(np.uint32), frames[-1][1].view(np.uint32)) and int(st.shadow_rays) == want[2]
        assert _counts(ctx) == (N_RANGES, 0, 2 * N_RANGES)
        ctx.close()
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1].view(np.uint32), frames[1][1].view(np.uint32))


# -------------------------------------------------------------------------------- 3. queries
@pytest.mark.parametrize("any_hit", [False, True])
def test_queries_on_device_built_trees_match_the_checker(any_hit):
    rig = BuildRig()
    objs = rig.meshes + [rig.marble]  # (no ground: in list order it would occlude every ANY query first)
    sc = LoweredScene(objs, [], Camera())
    rays = _query_rays()
    # ... and 9 rays through the repeated triangle, where every one of its 9 copies ties
    nine = rig.meshes[5].positions.astype(np.float64)
    targets = np.array([nine[0] * a + nine[1] * b + nine[2] * (1.0 - a - b) for a, b in
                        [(0.2, 0.2), (0.6, 0.2), (0.2, 0.6), (0.4, 0.3), (0.3, 0.4), (0.1, 0.1), (0.8, 0.1), (0.1, 0.8), (0.34, 0.33)]])
    origins = targets + np.array([0.3, 0.4, 9.0])
    extra = q.rays_of(origins.astype(F), (targets - origins).astype(F), q.T_MIN, q.INF)
    rays = np.concatenate([rays, extra])
    want = ir.any_hit(sc, rays) if any_hit else ir.closest(sc, rays)
    on_mesh = sum(sc.prims[i].kind == abi.PRIM_MESH for i in want["prim"][want["prim"] >= 0])
    assert on_mesh > 40, "the rays hardly touch the meshes"
    ctx = _device_ctx()
    got = _raycast(ctx, sc, rays, any_hit)
    q.assert_hits_equal(got, want, tri=True)
    assert (want["prim"][-9:] == 5).all()
    if not any_hit:  # the lowest original index wins the tie, although the slots are in sorted order
        assert (got["tri"][-9:] == 0).all()
    assert _counts(ctx) == (N_RANGES, 0, N_RANGES)
    ctx.close()


def test_a_mesh_beyond_one_sort_block_is_the_reference_tree_and_answers_queries():
    """icosphere(4), 5120 triangles: more keys than one workgroup of the radix sort takes."""
    ball = icosphere((0.5, 2.0, -1.0), 3.0, 4, _mat(0.8, 0.3, 0.3))
    assert ball.num_triangles == 5120
    sc = LoweredScene([ball], [], Camera())
    rays = _query_rays()
    want = ir.closest(sc, rays)
    assert (want["prim"] == 0).sum() > 100 and len(set(want["tri"][want["prim"] == 0].tolist())) > 80
    ctx = _device_ctx()
    q.assert_hits_equal(_raycast(ctx, sc, rays, False), want, tri=True)
    q.assert_hits_equal(_raycast(ctx, sc, rays, True), ir.any_hit(sc, rays), tri=True)
    assert _counts(ctx) == (1, 0, 1)
    ref = _assert_tree_is_the_reference(ctx, sc)
    assert len(ref["links"]) == 1279
    ctx.close()


# --------------------------------------------------------------- 4. refits, instances, in flight
def test_device_build_then_refits_a_moved_sphere_and_an_index_change():
    w, h = 64, 36
    rig = Rig()
    prm = cfg_of(w, h).lower()
    ctx = _device_ctx()
    sc0 = rig.scene()
    _check_frame(ctx, sc0, prm, _oracle_frame(("pose0", w, h, "lambert_shadow"), sc0, prm))
    built = ctx.mesh_nodes()
    slot_vtx = rr.slot_vertex_table(sc0, ctx.mesh_slots())
    assert _counts(ctx) == (4, 0, 4)
    for k in (1, 2):
        sc = rig.set_pose(k).scene()
        ctx.mesh_refit(sc)
        _check_frame(ctx, sc, prm, _oracle_frame((f"pose{k}", w, h, "lambert_shadow"), sc, prm))
        got = ctx.mesh_nodes()
        want, _ = rr.refit(built, slot_vtx, sc._mesh_vtx[:, :3])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        ri = ctx.refit_info()
        assert (ri.refits, ri.device_refits, ri.deformed) == (k, k, 1) and _counts(ctx) == (4, 0, 4)
    # only a sphere moves: a cache hit, nothing is built by either builder
    assert sc.prims[5].kind == abi.PRIM_SPHERE
    sc.prims[5].p[0], sc.prims[5].p[1], sc.prims[5].p[2] = -2.0, 0.7, 8.0
    _check_frame(ctx, sc, prm, _oracle_frame(("build-sphere", w, h), sc, prm))
    assert _counts(ctx) == (4, 0, 4) and ctx.refit_info().device_refits == 3
    # switching the policy alone rebuilds nothing
    ctx.set_mesh_build(HOST)
    _render(ctx, sc, prm)
    ctx.set_mesh_build(DEVICE)
    _render(ctx, sc, prm)
    assert _counts(ctx) == (4, 0, 4)
    # an index change (the fan's first triangle turned over): the refit is refused, the device builds again
    fan = rig.meshes[2]
    turned = fan.indices.copy()
    turned[0] = turned[0][::-1]
    rig.meshes[2] = Mesh(fan.positions, turned, None, fan.material)
    sc = rig.scene()
    with pytest.raises(abi.RrteError) as e:
        ctx.mesh_refit(sc)
    assert e.value.status == abi.RRTE_INVALID_ARG and "index" in str(e.value)
    _check_frame(ctx, sc, prm, _oracle_frame(("build-index", w, h), sc, prm))
    assert _counts(ctx) == (8, 0, 8) and ctx.refit_info().deformed == 0
    _assert_tree_is_the_reference(ctx, sc)
    ctx.close()


def test_instances_of_a_deformed_device_built_base(monkeypatch):
    w, h = 64, 36
    monkeypatch.setenv("RRTE_JIT_TOPO", "0")
    ball = icosphere((-4.0, 2.3, -3.0), 2.2, 2, _mat(0.8, 0.3, 0.3))
    base = ball.positions.copy()
    objs, lights = _family(ball, w, h), _lights()
    prm = cfg_of(w, h).lower()
    sc0 = LoweredScene(objs, lights, cam(w, h))
    ball.set_vertices(deform(base, 1))
    sc1 = LoweredScene(objs, lights, cam(w, h))
    assert [sc1.prims[i].kind for i in range(4)] == [0, 8, 9, 9] and sc1.prims[3].trs[7] < 0  # (one mirrored)
    want = _oracle_frame(("family", w, h), sc1, prm, lambda s, p, lin: ir.render(monkeypatch, s, p, linear=lin))
    ctx = _device_ctx()
    _touch(ctx, sc0)
    ctx.mesh_refit(sc1)
    _check_frame(ctx, sc1, prm, want, 0)
    mi = ctx.mesh_info()
    assert (mi.ranges, mi.tri_slots) == (1, 320) and _counts(ctx) == (1, 0, 1) and ctx.refit_info().device_refits == 1
    ctx.close()


def test_a_frame_in_flight_keeps_its_scene_while_the_next_is_built():
    import torch
    w, h = 64, 36
    rig = Rig().set_pose(1)
    prm = cfg_of(w, h).lower()
    sc_a = rig.scene()
    sc_b = rig.set_pose(2).scene()
    want_a = _oracle_frame(("pose1", w, h, "lambert_shadow"), sc_a, prm)
    want_b = _oracle_frame(("pose2", w, h, "lambert_shadow"), sc_b, prm)
    ctx = _device_ctx()
    buf = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rrte_hip_render_async(ctx.h, sc_a.ref(), C.byref(prm), buf.data_ptr(), None, None))
    got_b = _render(ctx, sc_b, prm, linear=False)[0]  # a cache miss: the device builds while frame a may run
    ctx.check(ctx.lib.rrte_hip_synchronize(ctx.h))
    got_a = buf.cpu().numpy().view(np.uint8)
    assert np.abs(got_a.astype(np.int16) - want_a[0].astype(np.int16)).max() <= 1
    assert np.abs(got_b.astype(np.int16) - want_b[0].astype(np.int16)).max() <= 1
    assert not np.array_equal(got_a, got_b) and _counts(ctx) == (8, 0, 8)
    ctx.close()


def test_emulated_peers_render_a_device_built_scene_exactly(monkeypatch):
    import torch
    w, h, nranks = 64, 36, 2
    rig = BuildRig()
    prm = cfg_of(w, h).lower()
    sc = rig.scene(w, h)
    ctx = _device_ctx()
    plain = np.zeros(w * h * 4, dtype=np.uint8)
    ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), plain.ctypes.data_as(C.POINTER(C.c_uint8))))
    ctx.close()
    assert len(np.unique(plain.reshape(-1, 4), axis=0)) > 100
    monkeypatch.setenv("RRTE_FORCE_GATHER", "1")
    monkeypatch.setenv("RRTE_EMULATE_PEERS", str(nranks))
    monkeypatch.setenv("RRTE_MESH_BUILD", "device")
    ctx = Context(0, jit=abi.JIT_OFF)
    lib = ctx.lib
    uid = (C.c_uint8 * abi.UNIQUE_ID_BYTES)()
    ctx.check(lib.rrte_hip_comm_unique_id(uid))
    ctx.check(lib.rrte_hip_comm_init(ctx.h, 1, 0, uid))
    out = torch.full((w * h,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(lib.rrte_hip_render_gather_async(ctx.h, sc.ref(), C.byref(prm), 0, out.data_ptr(), None))
    ctx.check(lib.rrte_hip_flush(ctx.h))
    ctx.check(lib.rrte_hip_synchronize(ctx.h))
    got = out.cpu().numpy().view(np.uint8)
    bad = got != plain
    assert not bad.any(), f"{int(bad.sum())} bytes differ from the plain render"
    assert _counts(ctx) == (N_RANGES, 0, N_RANGES)
    ctx.close()


def test_debug_check_word_stays_clear_after_a_device_build(monkeypatch):
    monkeypatch.setenv("RRTE_DEBUG", "4")
    rig = BuildRig()
    prm = cfg_of(64, 36).lower()
    ctx = _device_ctx()
    sc = rig.scene()
    _check_frame(ctx, sc, prm, _oracle_frame(("build", 64, 36, "lambert_shadow"), sc, prm))
    sc1 = rig.set_pose(1).scene()
    ctx.mesh_refit(sc1)
    _render(ctx, sc1, prm)
    assert _counts(ctx) == (N_RANGES, 0, N_RANGES) and ctx.refit_info().device_refits == 1
    word = C.c_uint64(99)
    ctx.check(ctx.lib.rrte_hip_check_word(ctx.h, C.byref(word)))
    assert word.value == 0
    ctx.close()


# ------------------------------------------------------------------------- 5. the depth boundary
def caterpillar(cluster):
    """4 triangles in each Morton cell 2^k (k = 0..29), 2 in the far corner (they pin the centroid box to
    [0, 1024]^3, so a centre's cell is its integer part), `cluster` triangles in cell 0, in shuffled
    index order.  Every triangle lies in a plane z = const with its box centred on a chosen point."""
    centres = [(0.0, 0.0, 0.0)] + [(0.25 + i / 128.0,) * 3 for i in range(1, cluster)]
    for k in range(30):
        axis, at = 2 - k % 3, float(1 << (k // 3)) + 0.5
        for i in range(4):
            c = [0.5 + i / 16.0] * 3
            c[axis] = at + i / 16.0
            centres.append(tuple(c))
    centres += [(1024.0, 1024.0, 1024.0), (1023.5, 1023.5, 1023.5)]
    c = np.array(centres, np.float64)
    d = 1.0 / 64.0
    corners = np.array([[-d, -d, 0.0], [d, -d, 0.0], [0.0, d, 0.0]])
    pos = (c[:, None, :] + corners[None, :, :]).reshape(-1, 3).astype(F)
    tris = np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)
    tris = tris[np.random.default_rng(7).permutation(len(tris))]
    return Mesh(pos, tris, None, _mat(0.6, 0.6, 0.2))


def _centroid_rays(mesh):
    """One ray per triangle, aimed at its centroid from the octant that holds no geometry."""
    p = mesh.positions.astype(np.float64)[mesh.indices.astype(np.int64)]
    target = p.mean(axis=1)
    dirn = np.array([0.31, 0.52, 0.8]) / np.linalg.norm([0.31, 0.52, 0.8])
    origins = target - 40.0 * dirn
    return q.rays_of(origins.astype(F), np.tile(dirn.astype(F), (len(target), 1)), q.T_MIN, q.INF)


@pytest.mark.parametrize("cluster", [32, 4])
def test_the_depth_boundary(cluster):
    mesh = caterpillar(cluster)
    sc = LoweredScene([mesh], [], Camera())
    ref = lr.build_scene(sc)
    codes = set(ref["ranges"][0]["codes"])
    assert codes == {0, (1 << 30) - 1} | {1 << k for k in range(30)}  # the input's precondition
    ctx = _device_ctx()
    rays = _centroid_rays(mesh)
    assert len(rays) == mesh.num_triangles == cluster + 122
    want = ir.closest(sc, rays)
    assert (want["prim"] == 0).all() and len(set(want["tri"].tolist())) > len(rays) // 2
    got = _raycast(ctx, sc, rays, False)
    q.assert_hits_equal(got, want, tri=True)
    bi = ctx.build_info()
    if cluster == 32:
        assert ref["depth"] == 33 > lr.MAX_RECORDS  # deeper than the traversal stack: the host builds
        assert _counts(ctx) == (0, 1, 1) and bi.depth == 0  # (no device build has happened)
    else:
        assert 30 <= ref["depth"] <= lr.MAX_RECORDS
        assert _counts(ctx) == (1, 0, 1) and bi.depth == ref["depth"] >= 30
        _assert_tree_is_the_reference(ctx, sc)
    ctx.close()


@pytest.mark.parametrize("named", [True, False])
def test_a_non_finite_vertex_falls_back_only_when_a_range_names_it(named):
    rig = Rig()
    tri = rig.meshes[3]
    p = tri.positions.copy()
    p[0 if named else 3, 1] = np.inf  # vertex 3 is the one nothing names
    tri.set_vertices(p, normals=tri.normals)
    sc = rig.scene()
    ctx = _device_ctx()
    _touch(ctx, sc)
    assert _counts(ctx) == ((0, 1, 4) if named else (4, 0, 4))
    if not named:
        prm = cfg_of(64, 36).lower()
        _check_frame(ctx, sc, prm, _oracle_frame(("build-inf-unnamed", 64, 36), sc, prm))
    ctx.close()


# -------------------------------------------------------------- 6. argument errors and plumbing
def test_bad_policy_values_and_the_environment_variable(monkeypatch):
    monkeypatch.delenv("RRTE_MESH_BUILD", raising=False)
    ctx = Context(0, jit=abi.JIT_OFF)
    assert ctx.build_info().policy == HOST
    for bad in (2, 7, 0xFFFFFFFF):
        with pytest.raises(abi.RrteError) as e:
            ctx.set_mesh_build(bad)
        assert e.value.status == abi.RRTE_INVALID_ARG and "policy" in str(e.value)
    bi = ctx.build_info()
    assert (bi.policy, bi.device_builds, bi.host_fallbacks, bi.depth) == (HOST, 0, 0, 0)
    rig = Rig()
    _touch(ctx, rig.scene())
    assert _counts(ctx) == (0, 0, 4)  # the default policy builds on the host and counts no fallback
    ctx.close()
    for value, policy in (("device", DEVICE), ("host", HOST), ("gpu", HOST), ("", HOST), ("1", HOST)):
        monkeypatch.setenv("RRTE_MESH_BUILD", value)
        ctx = Context(0, jit=abi.JIT_OFF)
        assert ctx.build_info().policy == policy, value
        ctx.close()
    monkeypatch.delenv("RRTE_MESH_BUILD")
    rt = Raytracer(cfg_of(64, 36), device=0, jit=abi.JIT_OFF, mesh_build=DEVICE)
    frame = rt.render(rig.objects(), rig.lights, [], cam(64, 36))
    assert _counts(rt.ctx) == (4, 0, 4)
    host = Raytracer(cfg_of(64, 36), device=0, jit=abi.JIT_OFF)
    assert np.array_equal(frame, host.render(rig.objects(), rig.lights, [], cam(64, 36))) and _counts(host.ctx) == (0, 0, 4)
    rt.ctx.close()
    host.ctx.close()


def test_cpp_mirror_builds_on_the_device(tmp_path):
    import oracle
    from rrte_amd import Color, LambertianMaterial, PointLight, RaytracerConfig, Sphere, scenes
    from rrte_amd.mesh import heightfield
    subprocess.run(["make", "-s", "-C", str(ROOT / "rrte_amd" / "cpp")], check=True)
    w, h = 64, 36
    field = heightfield((-3.0, 0.5, -2.0), 6.0, 7, lambda x, z: 0.6 * np.sin(x) * np.cos(z),
                        LambertianMaterial(Color(0.8, 0.3, 0.3, 1.0)))
    blob, out = tmp_path / "mesh.bin", tmp_path / "frame.bin"
    with open(blob, "wb") as f:
        f.write(np.array([len(field.positions), len(field.indices)], np.uint32).tobytes())
        f.write(field.positions.tobytes() + field.normals.tobytes() + field.indices.tobytes())
    subprocess.run([str(TOOL), "render", str(blob), str(w), str(h), str(out)], check=True)
    raw = out.read_bytes()
    before, after = abi.BuildInfo.from_buffer_copy(raw[:24]), abi.BuildInfo.from_buffer_copy(raw[24:48])
    assert (before.policy, before.device_builds, before.host_fallbacks, before.depth) == (DEVICE, 0, 0, 0)
    assert (after.policy, after.device_builds, after.host_fallbacks) == (DEVICE, 1, 0) and after.depth >= 4
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, LambertianMaterial(Color(0.5, 0.5, 0.5, 1.0))), field]
    lights = [PointLight((-10.0, 15.0, 10.0), Color(1.0, 1.0, 1.0, 1.0), 25.0)]
    sc = LoweredScene(objs, lights, scenes._camera(w, h, (1.0, 7.0, 16.0), (1.0, 1.5, 0.0)))
    cfg = RaytracerConfig(max_depth=1, samples_per_pixel=1, width=w, height=h, mode="lambert_shadow", jitter="center")
    r8, _, _ = oracle.render(sc, cfg.lower(), nthreads=8)
    got = np.frombuffer(raw[48:], np.uint8)
    assert len(got) == w * h * 4 and np.abs(got.astype(np.int16) - r8.astype(np.int16)).max() <= 1
