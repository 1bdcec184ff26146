"""The enclosure of the march clip (rrte_amd/csrc/march_clip.hpp, exported by rrte_hip_march_clip of
include/rrte_hip_clip.h) against the float64 reference of the SDF path (tests/sdf_f64.py), without a GPU.

A march of a ray (o, d) that ends at tend reports a hit only where f <= L = E tend + D, E = eps (1 + 2^-20),
D = 2^-17 (|o|_1 + tend + |cb|_1 + 4 R + K).  For every operator, k in {0, 0.05, 0.3, 0.8} and parts that are
disjoint, overlapping, tangent or nested, and for rays from near, far, inside the bounding sphere and
pointing away, every sampled point with f <= L must lie inside the enclosure the kernel would test that
ray against.  The samples hold points within 2^-8 of the enclosure's radius for every operator, found by
the float64 field alone (shells just under each part's grown radius and the seam a = b of a smooth union),
so an enclosure 0.4 % smaller fails.  Degenerate programs: a zero radius is enclosed like any other, a
negative radius and a smooth operator with k = 0 make the kernel stand down (RRTE_CLIP_NONE)."""
import numpy as np
import pytest

import sdf_f64
from rrte_amd import (Camera, CSGComposite, LambertianMaterial, Color, LoweredScene, SDFObject, SDFSphere, Sphere, abi,
                      to_radians)

OPS = ["union", "difference", "intersection", "smooth_union", "smooth_difference", "smooth_intersection"]
CLS = {"union": abi.CLIP_UNION, "smooth_union": abi.CLIP_UNION, "difference": abi.CLIP_DIFFERENCE,
       "smooth_difference": abi.CLIP_DIFFERENCE, "intersection": abi.CLIP_INTERSECTION,
       "smooth_intersection": abi.CLIP_INTERSECTION}
KS = [0.0, 0.05, 0.3, 0.8]
CA, RA = (0.0, 2.0, 0.0), 1.0
# part b beside part a (centre (0, 2, 0), radius 1)
LAYOUTS = {"disjoint": ((2.5, 2.0, 0.0), 0.7), "overlapping": ((0.6, 2.2, 0.0), 0.7), "tangent": ((1.7, 2.0, 0.0), 0.7),
           "nested": ((0.2, 2.0, 0.1), 0.4), "zero-radius-b": ((0.6, 2.2, 0.0), 0.0)}
# (origin, towards): near, far, from large coordinates, inside the bounding sphere, pointing away
RAYS = [((0.0, 8.0, 20.0), (0.3, 2.0, 0.0)), ((3.0, 2.5, 4.0), (0.9, 2.9, 0.0)), ((100.0, -50.0, 30.0), (0.5, 2.0, 0.0)),
        ((0.3, 3.2, 0.2), (2.0, 0.0, -1.0)), ((4.0, 3.0, 1.0), (9.0, 4.0, 2.0))]
MARGIN = 2.0 ** -8
RNG_SEED = 20240611


def _scene(op, k, cb, rb, ca=CA, ra=RA):
    mat = LambertianMaterial(Color.rgb(0.5, 0.5, 0.5))
    obj = SDFObject(CSGComposite(SDFSphere(ca, ra), SDFSphere(cb, rb), op, k), mat)
    cam = Camera.new_perspective(to_radians(50.0), 1.5, 0.1, 100.0)
    return LoweredScene([Sphere((0.0, -1000.0, 0.0), 1000.0, mat), obj], [], cam)


def _info(sc, i=1):
    info = abi.ClipInfo()
    assert abi.load().rrte_hip_march_clip(sc.ref(), i, info) == abi.RRTE_OK
    return info


def _unit_directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _samples(rng, pr, parts, k, smooth_union, level):
    """Points in the bounding sphere, shells just under each part's exact sublevel radius r (+ k/4) + level,
    and for a smooth union the seam a = b at that depth."""
    cb, R = np.array(pr.p[0:3], np.float64), float(pr.p[3])
    pts = [cb + R * _unit_directions(rng, 6000) * rng.uniform(0.0, 1.0, (6000, 1)) ** (1.0 / 3.0)]
    grow = 0.25 * k if smooth_union else 0.0
    for c, r in parts:
        for under in (1e-6, 0.5 * level, 1e-3):
            pts.append(np.array(c) + (r + grow + level - under) * _unit_directions(rng, 2500))
    if smooth_union:
        (c0, r0), (c1, r1) = parts
        c0, c1 = np.array(c0), np.array(c1)
        dist = np.linalg.norm(c1 - c0)
        s = grow + level - 1e-6  # a = b = s: the circle where the balls of radius r + s meet
        ra_, rb_ = r0 + s, r1 + s
        if dist > 0.0 and abs(ra_ - rb_) < dist < ra_ + rb_:
            x = (dist * dist + ra_ * ra_ - rb_ * rb_) / (2.0 * dist)
            rad = np.sqrt(max(ra_ * ra_ - x * x, 0.0))
            axis = (c1 - c0) / dist
            u = np.cross(axis, [0.0, 0.0, 1.0] if abs(axis[2]) < 0.9 else [1.0, 0.0, 0.0])
            u /= np.linalg.norm(u)
            w = np.cross(axis, u)
            ang = rng.uniform(0.0, 2.0 * np.pi, (2500, 1))
            pts.append(c0 + x * axis + rad * (np.cos(ang) * u + np.sin(ang) * w))
    return np.concatenate(pts)


def _check_family(op, k, layout, near):
    """near[op] collects how many in-region points lay within MARGIN of an enclosure radius."""
    cb_, rb_ = LAYOUTS[layout]
    sc = _scene(op, k, cb_, rb_)
    info, pr = _info(sc), sc.prims[1]
    smooth = op.startswith("smooth")
    if smooth and k == 0.0:
        assert info.cls == abi.CLIP_NONE  # smin's 0/0 at a = b: the kernel stands down
        return
    assert info.cls == CLS[op], (op, k, layout)
    prog = sdf_f64.program(sc.nodes, pr.sdf_first, 3)
    parts = [(tuple(prog[0].f[0:3]), prog[0].f[3]), (tuple(prog[1].f[0:3]), prog[1].f[3])]
    kk = prog[2].f[0] if smooth else 0.0
    cbound, R = np.array(pr.p[0:3], np.float64), float(pr.p[3])
    E = float(pr.sdf_hit_eps) * (1.0 + 2.0 ** -20)
    K = max(sum(abs(v) for v in prog[0].f[0:7]), sum(abs(v) for v in prog[1].f[0:7])) + abs(prog[2].f[0])
    rng = np.random.default_rng(RNG_SEED)
    centres = [np.array(info.a_center[:], np.float64), np.array(info.b_center[:], np.float64)]
    assert np.array_equal(centres[0], parts[0][0]) and np.array_equal(centres[1], parts[1][0])
    for origin, towards in RAYS:
        o = np.array(origin, np.float64)
        d = np.array(towards, np.float64) - o
        d /= np.linalg.norm(d)
        # the march's end: the far crossing of the bounding sphere (a ray that misses it never marches:
        # take the sphere's far side), and the L of that march
        oc = o - cbound
        b = oc @ d
        tend = -b + np.sqrt(max(b * b - (oc @ oc - R * R), 0.0)) if b * b >= oc @ oc - R * R else np.linalg.norm(oc) + R
        tend = max(tend, 0.0)
        L = E * tend + 2.0 ** -17 * (np.abs(o).sum() + tend + np.abs(cbound).sum() + 4.0 * R + K)
        rho = [c0 + info.c1 * abs((o - c) @ d) + info.c2 * np.abs(o).sum() for c, c0 in zip(centres, (info.a_c0, info.b_c0))]
        pts = _samples(rng, pr, parts, kk, op == "smooth_union", L)
        f = sdf_f64.evaluate(prog, pts)
        region = pts[f <= L]  # (empty for an intersection of disjoint parts)
        rel = [np.linalg.norm(region - c, axis=1) / r for c, r in zip(centres, rho)]
        if info.cls == abi.CLIP_DIFFERENCE:
            inside, edge = rel[0] <= 1.0, rel[0]
        elif info.cls == abi.CLIP_INTERSECTION:
            inside, edge = (rel[0] <= 1.0) & (rel[1] <= 1.0), np.maximum(rel[0], rel[1])
        else:
            inside, edge = (rel[0] <= 1.0) | (rel[1] <= 1.0), np.minimum(rel[0], rel[1])
        assert inside.all(), (op, k, layout, origin, float(edge.max()))
        near[op] = near.get(op, 0) + int((edge >= 1.0 - MARGIN).sum())


def test_every_point_a_march_can_hit_lies_inside_the_enclosure():
    near = {}
    for op in OPS:
        for k in KS:
            for layout in LAYOUTS:
                _check_family(op, k, layout, near)
    print("in-region points within 2^-8 of an enclosure radius, by operator:", near)
    # not vacuous: every operator had points of its hit region just inside the enclosure
    assert all(near.get(op, 0) >= 100 for op in OPS), near


@pytest.mark.parametrize("op", OPS)
def test_a_negative_radius_stands_down(op):
    for cb, rb, ca, ra in (((0.6, 2.2, 0.0), -0.7, CA, RA), ((0.6, 2.2, 0.0), 0.7, CA, -1.0)):
        assert _info(_scene(op, 0.3, cb, rb, ca, ra)).cls == abi.CLIP_NONE


def test_other_objects_are_not_clipped():
    """The ground sphere, and a program that is not "sphere, sphere, operator"."""
    from rrte_amd import SDFBox
    mat = LambertianMaterial(Color.rgb(0.5, 0.5, 0.5))
    cam = Camera.new_perspective(to_radians(50.0), 1.5, 0.1, 100.0)
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, mat), SDFObject(SDFSphere(CA, RA), mat),
            SDFObject(CSGComposite(SDFSphere(CA, RA), SDFBox((0.5, 2.0, 0.0), (1.0, 1.0, 1.0)), "union", 0.0), mat)]
    sc = LoweredScene(objs, [], cam)
    for i in range(3):
        assert _info(sc, i).cls == abi.CLIP_NONE
    info = abi.ClipInfo()
    assert abi.load().rrte_hip_march_clip(sc.ref(), 3, info) == abi.RRTE_INVALID_ARG
    assert abi.load().rrte_hip_march_clip(None, 0, info) == abi.RRTE_INVALID_ARG


def test_the_header_and_the_binding_agree():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parents[1] / "include" / "rrte_hip_clip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(rrte_hip_\w+)\s*\(", code)) == set(abi.CLIP_EXPORTS)
    consts = dict(re.findall(r"#define (RRTE_CLIP_\w+)\s+(\d+)u", code))
    assert consts == {"RRTE_CLIP_NONE": "0", "RRTE_CLIP_DIFFERENCE": "1", "RRTE_CLIP_INTERSECTION": "2", "RRTE_CLIP_UNION": "4"}
    for other in (abi.EXPORTS, abi.QUERY_EXPORTS, abi.MESH_EXPORTS, abi.REFIT_EXPORTS, abi.BUILD_EXPORTS, abi.ACCEL_EXPORTS,
                  abi.JIT_EXPORTS):
        assert not set(abi.CLIP_EXPORTS) & set(other)
