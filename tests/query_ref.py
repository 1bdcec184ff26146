"""Checker side of the ray-query tests (tests/test_gpu_query.py): the fixed ray generator and the
loop over rrte_oracle_intersect that defines what a query must return (include/rrte_hip_query.h).
CPU only; nothing here touches the device."""
import ctypes as C
import functools

import numpy as np

import oracle
from rrte_amd import abi

N_RAYS = 517  # 8 waves plus a 5-lane tail
T_MIN = np.float32(1e-3)
INF = np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def gen_rays(n=N_RAYS):
    """(origins, directions, |target - origin|): origins uniform in [-12,12]x[0.2,9]x[-12,12], targets
    uniform in [-8,8]x[0,4]x[-8,8], direction = (target - origin) * s with s uniform in [0.1, 3] --
    deliberately not unit length.  Read-only float32 arrays."""
    rng = np.random.default_rng(0x5EED2025)
    o = rng.uniform([-12.0, 0.2, -12.0], [12.0, 9.0, 12.0], (n, 3)).astype(np.float32)
    tg = rng.uniform([-8.0, 0.0, -8.0], [8.0, 4.0, 8.0], (n, 3)).astype(np.float32)
    s = rng.uniform(0.1, 3.0, n).astype(np.float32)
    seg = tg - o
    d = seg * s[:, None]
    length = np.sqrt((seg.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    for a in (o, d, length):
        a.setflags(write=False)
    return o, d, length


def rays_of(origins, directions, t_min=T_MIN, t_max=INF):
    rays = np.zeros(len(origins), dtype=abi.RAY_DTYPE)
    rays["origin"], rays["direction"] = origins, directions
    rays["t_min"], rays["t_max"] = t_min, t_max
    return rays


def miss_record():
    h = np.zeros((), dtype=abi.RAY_HIT_DTYPE)
    h["t"], h["prim"], h["material"] = INF, -1, -1
    return h


def _intersect(lib, sc, i, ray, t_max, hit):
    return lib.rrte_oracle_intersect(C.byref(sc.ir), i, oracle.farr(ray["origin"]), oracle.farr(ray["direction"]),
                                     float(ray["t_min"]), float(t_max), C.byref(hit))


def oracle_closest(sc, rays):
    """ray_color's search (raytracer.rs:103-113) with each ray's own interval: the objects in list
    order through rrte_oracle_intersect, strict '<'; an SDF object gets min(t_max, best.t) once a hit
    exists.  Returns RAY_HIT_DTYPE records (tri left 0: the oracle has no mesh triangle index)."""
    lib = oracle.load()
    n_prims = sc.ir.num_prims
    kinds = [sc.prims[i].kind for i in range(n_prims)]
    mats = [sc.prims[i].material for i in range(n_prims)]
    out = np.zeros(len(rays), dtype=abi.RAY_HIT_DTYPE)
    for k, ray in enumerate(rays):
        best, best_i = None, -1
        for i in range(n_prims):
            t_max = np.float32(ray["t_max"])
            if kinds[i] == abi.PRIM_SDF and best is not None:
                t_max = t_max if t_max < np.float32(best.t) else np.float32(best.t)
            h = oracle.OracleHit()
            if _intersect(lib, sc, i, ray, t_max, h) and (best is None or h.t < best.t):
                best, best_i = h, i
        if best is None:
            out[k] = miss_record()
        else:
            out[k]["t"], out[k]["prim"], out[k]["material"] = best.t, best_i, mats[best_i]
            out[k]["point"], out[k]["normal"] = list(best.point), list(best.normal)
            out[k]["front_face"] = 1 if best.front_face else 0
    return out


def oracle_any(sc, rays):
    """RRTE_QUERY_ANY: prim = the lowest index whose rrte_oracle_intersect reports a hit in
    [t_min, t_max], material = its material, everything else zero; a miss is prim = material = -1."""
    lib = oracle.load()
    out = np.zeros(len(rays), dtype=abi.RAY_HIT_DTYPE)
    out["prim"], out["material"] = -1, -1
    for k, ray in enumerate(rays):
        for i in range(sc.ir.num_prims):
            if _intersect(lib, sc, i, ray, ray["t_max"], oracle.OracleHit()):
                out[k]["prim"], out[k]["material"] = i, sc.prims[i].material
                break
    return out


def _ray_new_direction(v):
    """Ray::new's normalisation (ray.rs:13-18; glam: v * (1 / sqrt(v.v))) of (n, 3) float32 rows."""
    v = v.astype(np.float32)
    x = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return v * (np.float32(1.0) / np.sqrt(x))[:, None]


def oracle_pick_rays(sc, w, h, xs, ys, t_min):
    """The pixel-centre camera rays of the frame kernel and the oracle's render: u = (x + 0.5) / w and
    v = (y + 0.5) / h in f32, through rrte_oracle_generate_ray.

    rrte_oracle_intersect builds its ray with Ray::new, which normalises the direction once more, and
    normalising is not idempotent in f32 (one pixel in five of the perspective frames used here moves
    by an ulp).  So the record's direction is not the camera ray's d itself but a positive multiple D
    of it that Ray::new maps back to d bit for bit -- found by a deterministic search and asserted --
    and the oracle loop then tests exactly the frame's primary ray."""
    lib = oracle.load()
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    rays = np.zeros(len(xs), dtype=abi.RAY_DTYPE)
    for k, (x, y) in enumerate(zip(xs, ys)):
        u = (np.float32(x) + np.float32(0.5)) / np.float32(w)
        v = (np.float32(y) + np.float32(0.5)) / np.float32(h)
        lib.rrte_oracle_generate_ray(C.byref(sc.ir.camera), float(u), float(v), o, d)
        rays[k]["origin"], rays[k]["direction"] = list(o), list(d)
    want = np.ascontiguousarray(rays["direction"])
    found = want.copy()
    todo = (_ray_new_direction(found).view(np.uint32) != want.view(np.uint32)).any(axis=1)
    for j in range(1, 1 << 14):
        if not todo.any():
            break
        cand = (want[todo] * (np.float32(1.0) + np.float32(j) * np.float32(2.0 ** -12))).astype(np.float32)
        ok = (_ray_new_direction(cand).view(np.uint32) == want[todo].view(np.uint32)).all(axis=1)
        idx = np.flatnonzero(todo)[ok]
        found[idx] = cand[ok]
        todo[idx] = False
    assert not todo.any(), "no direction normalises to the camera ray"
    assert np.array_equal(_ray_new_direction(found).view(np.uint32), want.view(np.uint32))
    rays["direction"] = found
    rays["t_min"], rays["t_max"] = t_min, INF
    return rays


def assert_hits_equal(got, want, tri=False):
    """prim, front_face and material equal; t, point and normal bit-identical as uint32, a NaN on both
    sides counting as equal."""
    assert got.shape == want.shape
    fields = ["prim", "front_face", "material", "_pad"] + (["tri"] if tri else [])
    for f in fields:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (f, bad[:5], got[bad[:5]], want[bad[:5]])
    for f in ("t", "point", "normal"):
        g = np.ascontiguousarray(got[f]).reshape(len(got), -1)
        w = np.ascontiguousarray(want[f]).reshape(len(want), -1)
        same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
        bad = np.flatnonzero(~same.all(axis=1))
        assert bad.size == 0, (f, bad[:5], got[bad[:5]], want[bad[:5]])
