"""Checker for mesh instances (RRTE_PRIM_MESH_INSTANCE, include/rrte_hip.h) -- TEST ONLY, CPU only.

Built from what exists: numpy_ref's f32 matrix helpers (bit-identical to the device for the
transformed analytic kinds) and rrte_oracle_intersect on a scene that holds the instance's BASE range
as a plain RRTE_PRIM_MESH.  Per ray: form the local ray, `len` and the local interval in f32 as the
header spells them out, ask the oracle for the base's hit, recover the unflipped normal from the
oracle's normal and front_face, and apply step 6 (t = tl / len, point through M, normal through the
inverse transpose, HitInfo::new against the world ray).

`patch_numpy_ref(monkeypatch, scene)` makes numpy_ref.render call this checker for kinds 8 and 9 and
its stock intersect otherwise, which gives the linear image and the shadow-ray count of a frame;
`closest` / `any_hit` give ray-query records.
"""
import ctypes as C

import numpy as np

import numpy_ref as nr
import oracle
import query_ref as q
from rrte_amd import abi

F = np.float32
INF = F(np.inf)
MESH_KINDS = (abi.PRIM_MESH, abi.PRIM_MESH_INSTANCE)


class BaseScenes:
    """Scenes of ONE plain kind-8 prim over (a sub-range of) the mesh arrays of `ir`, by range."""

    def __init__(self, ir):
        self.ir = ir
        self._cache = {}

    def get(self, first, count):
        key = (int(first), int(count))
        if key not in self._cache:
            prims = (abi.Prim * 1)()
            prims[0].kind = abi.PRIM_MESH
            prims[0].material = -1
            prims[0].sdf_first, prims[0].sdf_count = key
            prims[0].trs[6] = 1.0
            prims[0].trs[7] = prims[0].trs[8] = prims[0].trs[9] = 1.0
            ir = abi.SceneIR()
            ir.prims, ir.num_prims = prims, 1
            ir.mesh_vertices, ir.num_mesh_vertices = self.ir.mesh_vertices, self.ir.num_mesh_vertices
            ir.mesh_indices, ir.num_mesh_indices = self.ir.mesh_indices, self.ir.num_mesh_indices
            ir.camera = self.ir.camera
            self._cache[key] = (ir, prims)
        return self._cache[key][0]


def normalize_rows(v):
    """Ray::new's normalisation of (n, 3) float32 rows (glam: v * (1 / sqrt(v.v)))."""
    return q._ray_new_direction(np.asarray(v, dtype=F))


def pre_normalised(want):
    """(n, 3) float32 directions D that Ray::new maps to `want` bit for bit: rrte_oracle_intersect
    normalises the direction it is given, and normalising is not idempotent in f32, so a ray whose
    direction is already final is handed over as a positive multiple of it, or of a neighbour a few
    ulps away, that normalises back to it (the search of query_ref.oracle_pick_rays, widened: a
    direction that came out of a normalisation has a preimage, but not always among its own
    multiples).  Rows with a non-finite component stay as they are."""
    want = np.ascontiguousarray(want, dtype=F)
    found = want.copy()
    with np.errstate(all="ignore"):
        todo = (normalize_rows(found).view(np.uint32) != want.view(np.uint32)).any(axis=1)
        todo &= np.isfinite(want).all(axis=1)
        for j in range(1, 1 << 14):
            if not todo.any():
                break
            cand = (want[todo] * (F(1.0) + F(j) * F(2.0 ** -12))).astype(F)
            ok = (normalize_rows(cand).view(np.uint32) == want[todo].view(np.uint32)).all(axis=1)
            idx = np.flatnonzero(todo)[ok]
            found[idx] = cand[ok]
            todo[idx] = False
        # a direction that came out of a normalisation has a preimage, but not always among its own
        # multiples: also try its neighbours, every component up to two ulps away
        if todo.any():
            bits = want.view(np.int32)
            for dx in range(-2, 3):
                for dy in range(-2, 3):
                    for dz in range(-2, 3):
                        if not todo.any():
                            break
                        # (stepping the bit pattern of a finite, non-zero float moves it by ulps)
                        step = np.array([dx, dy, dz], np.int32) * np.where(bits[todo] < 0, -1, 1).astype(np.int32)
                        near = (bits[todo] + step).view(F)
                        for j in range(0, 64):
                            cand = (near * (F(1.0) + F(j) * F(2.0 ** -12))).astype(F)
                            ok = (normalize_rows(cand).view(np.uint32) == want[todo].view(np.uint32)).all(axis=1)
                            idx = np.flatnonzero(todo)[ok]
                            found[idx] = cand[ok]
                            todo[idx] = False
                            if not todo.any():
                                break
                            near = near[~ok]
    assert not todo.any(), "no direction normalises to the ray's"
    return found


def _oracle_rows(ir, o, d, tmin, tmax):
    """rrte_oracle_intersect of prim 0 of `ir` for every row: (ok, t, point (n,3), normal (n,3), front)."""
    lib = oracle.load()
    n = len(o)
    ok = np.zeros(n, bool)
    t = np.full(n, np.inf, F)
    p, nn = np.zeros((n, 3), F), np.zeros((n, 3), F)
    front = np.zeros(n, bool)
    tmin = np.broadcast_to(np.asarray(tmin, F), (n,))
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,))
    h = oracle.OracleHit()
    ref = C.byref(ir)
    for k in range(n):
        if lib.rrte_oracle_intersect(ref, 0, oracle.farr(o[k]), oracle.farr(d[k]), float(tmin[k]), float(tmax[k]),
                                     C.byref(h)):
            ok[k], t[k], front[k] = True, h.t, bool(h.front_face)
            p[k], nn[k] = list(h.point), list(h.normal)
    return ok, t, p, nn, front


def mesh_rows(bases, pr, o, d, tmin, tmax):
    """One kind-8 or kind-9 prim against n rays whose directions `d` are FINAL (already through
    Ray::new): (ok, t, point, normal, front, local) with the normal flipped towards the world ray;
    `local` = (local origin, direction to hand to the oracle, local t, local tmin, local tmax), what
    `triangle_index` needs."""
    o = np.ascontiguousarray(o, dtype=F)
    d = np.ascontiguousarray(d, dtype=F)
    n = len(o)
    tmin = np.broadcast_to(np.asarray(tmin, F), (n,)).astype(F)
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,)).astype(F)
    base = bases.get(pr.sdf_first, pr.sdf_count)
    if pr.kind == abi.PRIM_MESH:
        dd = pre_normalised(d)
        ok, t, p, nn, front = _oracle_rows(base, o, dd, tmin, tmax)
        return ok, t, p, nn, front, (o, dd, t, tmin, tmax)
    assert pr.kind == abi.PRIM_MESH_INSTANCE
    with np.errstate(all="ignore"):
        m = nr.mat4_srt(list(pr.trs))
        inv = nr.mat4_inverse(m)
        oc, dc = [o[:, k] for k in range(3)], [d[:, k] for k in range(3)]
        v = nr.m_vector(inv, dc)                                   # 1. v = m_vector(inv, r.d)
        ln = np.sqrt(nr.dot(v, v)).astype(F)                       # 2. len
        ld1 = nr.normalize(v)                                      # 3. vnorm(v); the oracle's Ray::new is ray_new's
        ld = nr.normalize(ld1)
        lo = nr.m_point(inv, oc)
        ltmin = (tmin * ln).astype(F)                              # 4. [t_min * len, t_max * len]
        ltmax = np.where(tmax == INF, INF, tmax * ln).astype(F)
        lo_r, ld1_r = np.stack(lo, 1).astype(F), np.stack(ld1, 1).astype(F)
        ok, tl, _, nn, lfront = _oracle_rows(base, lo_r, ld1_r, ltmin, ltmax)  # 5. the base's hit
        nl = np.where(lfront[:, None], nn, -nn)                    # the unflipped interpolated normal
        t = (tl / ln).astype(F)                                    # 6. t = tl / len
        lp = nr.at(lo, ld, tl)
        p = np.stack(nr.m_point(m, lp), 1).astype(F)
        nlc = [nl[:, k] for k in range(3)]
        nw = [nr.dot([inv[4 * j + 0], inv[4 * j + 1], inv[4 * j + 2]], nlc) for j in range(3)]
        nwn = np.stack(nr.normalize(nw), 1).astype(F)
        front = nr.dot(dc, [nwn[:, k] for k in range(3)]) < F(0)   # HitInfo::new against the WORLD ray
        nout = np.where(front[:, None], nwn, -nwn)
    t = np.where(ok, t, INF).astype(F)
    return ok, t, p, nout, front, (lo_r, ld1_r, tl, ltmin, ltmax)


def triangle_index(bases, pr, local, rows):
    """The index within the prim's range of the triangle that wins each of `rows` (hit rays): the lowest
    index whose own test reports the winning local t (strict '<': the lower index wins a tie)."""
    lo, ld, tl, ltmin, ltmax = local
    lib = oracle.load()
    out = np.zeros(len(rows), np.uint32)
    h = oracle.OracleHit()
    for j, k in enumerate(rows):
        want = np.float32(tl[k]).view(np.uint32)
        for tri in range(pr.sdf_count):
            one = bases.get(pr.sdf_first + tri, 1)
            if lib.rrte_oracle_intersect(C.byref(one), 0, oracle.farr(lo[k]), oracle.farr(ld[k]), float(ltmin[k]),
                                         float(ltmax[k]), C.byref(h)) and np.float32(h.t).view(np.uint32) == want:
                out[j] = tri
                break
        else:
            raise AssertionError(f"no triangle of the range reports t = {tl[k]!r}")
    return out


# ------------------------------------------------------------------------------------ frames
def patch_numpy_ref(monkeypatch, ir):
    """numpy_ref.render of `ir` (an abi.SceneIR) with mesh objects: kinds 8 and 9 go through this
    checker, every other kind through the stock numpy_ref.intersect."""
    bases = BaseScenes(ir)
    stock = nr.intersect

    def intersect(pr, o, d, tmin, tmax, nodes=None):
        if pr.kind not in MESH_KINDS:
            return stock(pr, o, d, tmin, tmax, nodes)
        ok, t, p, nn, _, _ = mesh_rows(bases, pr, np.stack(o, 1), np.stack(d, 1), tmin, tmax)
        h = nr.Hits(len(ok))
        h.ok, h.t = ok, t
        h.p = [p[:, k] for k in range(3)]
        h.n = [nn[:, k] for k in range(3)]
        return h

    monkeypatch.setattr(nr, "intersect", intersect)


def render(monkeypatch, scene, params, linear=True):
    """numpy_ref.render of a LoweredScene with mesh objects: (rgba8, f32, shadow rays)."""
    patch_numpy_ref(monkeypatch, scene.ir)
    return nr.render(scene.ir, params, linear=linear)


# ----------------------------------------------------------------------------------- queries
def _prim_rows(sc, bases, i, rays, d_final, tmax):
    """Prim i against the query rays: (ok, t, point, normal, front, tri or None)."""
    pr = sc.prims[i]
    if pr.kind in MESH_KINDS:
        ok, t, p, nn, front, local = mesh_rows(bases, pr, rays["origin"], d_final, rays["t_min"], tmax)
        return ok, t, p, nn, front, (pr, local)
    lib = oracle.load()
    n = len(rays)
    ok, t = np.zeros(n, bool), np.full(n, np.inf, F)
    p, nn, front = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros(n, bool)
    h = oracle.OracleHit()
    for k, ray in enumerate(rays):
        if lib.rrte_oracle_intersect(C.byref(sc.ir), i, oracle.farr(ray["origin"]), oracle.farr(ray["direction"]),
                                     float(ray["t_min"]), float(tmax[k]), C.byref(h)):
            ok[k], t[k], front[k] = True, h.t, bool(h.front_face)
            p[k], nn[k] = list(h.point), list(h.normal)
    return ok, t, p, nn, front, None


def closest(sc, rays):
    """RRTE_QUERY_CLOSEST records (query_ref.oracle_closest's rule: list order, strict '<', an SDF
    object marches up to min(t_max, best t)), with mesh objects through this checker and `tri` filled."""
    n = len(rays)
    bases = BaseScenes(sc.ir)
    with np.errstate(all="ignore"):
        d_final = normalize_rows(rays["direction"])
    out = np.zeros(n, dtype=abi.RAY_HIT_DTYPE)
    out[:] = q.miss_record()
    best_t = np.full(n, np.inf, F)
    found = np.zeros(n, bool)
    tri_src = {}
    for i in range(sc.ir.num_prims):
        tmax = rays["t_max"].astype(F)
        if sc.prims[i].kind == abi.PRIM_SDF:
            tmax = np.where(found & (best_t < tmax), best_t, tmax).astype(F)
        ok, t, p, nn, front, mesh = _prim_rows(sc, bases, i, rays, d_final, tmax)
        with np.errstate(invalid="ignore"):
            better = ok & (~found | (t < best_t))
        out["t"][better], out["prim"][better] = t[better], i
        out["point"][better], out["normal"][better] = p[better], nn[better]
        out["front_face"][better] = front[better]
        out["material"][better] = sc.prims[i].material
        best_t = np.where(better, t, best_t)
        found |= better
        if mesh is not None:
            tri_src[i] = mesh
    out["tri"] = 0
    for i, (pr, local) in tri_src.items():
        rows = np.flatnonzero(out["prim"] == i)
        if rows.size:
            out["tri"][rows] = triangle_index(bases, pr, local, rows)
    return out


def any_hit(sc, rays):
    """RRTE_QUERY_ANY records: the lowest index whose test reports a hit in [t_min, t_max]."""
    n = len(rays)
    bases = BaseScenes(sc.ir)
    with np.errstate(all="ignore"):
        d_final = normalize_rows(rays["direction"])
    out = np.zeros(n, dtype=abi.RAY_HIT_DTYPE)
    out["prim"], out["material"] = -1, -1
    for i in range(sc.ir.num_prims):
        ok = _prim_rows(sc, bases, i, rays, d_final, rays["t_max"].astype(F))[0]
        first = ok & (out["prim"] < 0)
        out["prim"][first], out["material"][first] = i, sc.prims[i].material
    return out
