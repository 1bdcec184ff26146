"""Checker side of the frame-AOV tests (tests/test_gpu_aov.py): every plane of include/rrte_hip_aov.h
built from the records of the oracle loop -- query_ref.oracle_closest over query_ref.oracle_pick_rays,
the rule rrte_hip_pick documents -- plus the scene's materials and the background.  CPU only; nothing
here touches the device."""
import numpy as np

import query_ref as q
from rrte_amd import abi

PLANES = list(abi.AOV_PLANES)  # depth, prim, material, tri, normal, position, albedo: bit order
MESH_KINDS = (abi.PRIM_MESH, abi.PRIM_MESH_INSTANCE)


def pick_records(sc, w, h, t_min, pixels=None, closest=q.oracle_closest):
    """The RAY_HIT_DTYPE record of every pixel of the w x h frame of `sc`, row-major -- or of the
    (x, y) pairs `pixels` alone.  `closest`: the oracle loop (instance_ref.closest for a scene with
    mesh instances, which the C oracle does not know)."""
    if pixels is None:
        ys, xs = (a.ravel() for a in np.mgrid[0:h, 0:w])
    else:
        xs, ys = np.asarray(pixels).reshape(-1, 2).T
    return closest(sc, q.oracle_pick_rays(sc, w, h, xs, ys, t_min))


def planes_of(sc, records, background, shape=None):
    """{plane: array} of `records` (n RAY_HIT_DTYPE records): shape (n,) / (n, 4), or with `shape` =
    (h, w) reshaped to (h, w) / (h, w, 4).  ALBEDO: the material's albedo, zero for a material index
    outside the scene's materials, the background on a miss."""
    n = len(records)
    hit = records["prim"] >= 0
    out = {"depth": records["t"].astype("<f4"), "prim": records["prim"].astype("<i4"),
           "material": records["material"].astype("<i4"), "tri": records["tri"].astype("<u4")}
    normal = np.zeros((n, 4), "<f4")
    normal[:, :3] = records["normal"]
    normal[:, 3] = records["front_face"] != 0
    position = np.zeros((n, 4), "<f4")
    position[:, :3] = records["point"]
    position[:, 3] = hit
    albedo = np.zeros((n, 4), "<f4")
    albedo[~hit] = np.asarray(background, "<f4")
    mats = np.array([list(sc.mats[i].albedo) for i in range(sc.ir.num_materials)], "<f4").reshape(-1, 4)
    has_mat = hit & (records["material"] >= 0) & (records["material"] < len(mats))
    albedo[has_mat] = mats[records["material"][has_mat]]
    out.update(normal=normal, position=position, albedo=albedo)
    if shape is not None:
        out = {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def on_mesh(sc, prim):
    """Where `prim` (any shape) names a mesh or a mesh instance: the pixels whose TRI the C oracle
    cannot give."""
    kinds = np.array([sc.prims[i].kind for i in range(sc.ir.num_prims)])
    return (prim >= 0) & np.isin(kinds[np.maximum(prim, 0)], MESH_KINDS)


def sub_block(planes, rect):
    x0, y0, w, h = rect
    return {k: v[y0:y0 + h, x0:x0 + w] for k, v in planes.items()}


def assert_planes_equal(got, want, names=None, skip_tri=None):
    """Every plane bit-identical as uint32, a NaN on both sides counting as equal
    (query_ref.assert_hits_equal's rule).  `skip_tri`: a mask of pixels whose TRI is not compared."""
    for name in (names if names is not None else want):
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        same = g.view(np.uint32) == w.view(np.uint32)
        if g.dtype.kind == "f":
            same |= np.isnan(g) & np.isnan(w)
        if name == "tri" and skip_tri is not None:
            same |= skip_tri
        bad = np.argwhere(~same)
        assert bad.size == 0, (name, len(bad), bad[:5], g[tuple(bad[:5].T)], w[tuple(bad[:5].T)])
