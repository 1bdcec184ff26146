"""Scenes for the grouped object searches of the scene-specialised kernels (rrte_amd/csrc/search_groups.hpp).

One family: a ground sphere at index 0, one occluder hovering over the middle of the picture at a chosen
index, and small fillers on a ring around it that shadow only the ground beside themselves.  The probe
region -- the ground under the occluder -- is shadowed by the occluder alone, so a search that steps over
the occluder's group wrongly shows as a missing shadow.  Spheres and one-leaf SDF objects are mixed: the
occluder is an SDF sphere when `sdf_occluder`, every fifth filler an SDF box.  A scene of one object is a
standing SDF ring, which shadows its own inner side."""
import math
import re
from pathlib import Path

from rrte_amd import (AmbientLight, Camera, Color, DirectionalLight, LambertianMaterial, PointLight,
                      RaytracerConfig, SDFBox, SDFObject, SDFRing, SDFSphere, Sphere, to_radians)
from rrte_amd.math import f32, vec3

HEADER = Path(__file__).resolve().parents[1] / "rrte_amd" / "csrc" / "search_groups.hpp"
# objects per group: the header's default
GROUP = int(re.search(r"^#define RRTE_SEARCH_GROUPS (\d+)", HEADER.read_text(), re.M).group(1))


def lights_of(kind):
    """"L1" and "ring": one point light.  "L4": point, ambient, a directional light whose direction is no unit
    vector (the shadow cull never culls for it: an all-ones mask), a second point light."""
    if kind == "ring":  # nearly in the ring's plane: its top shadows the inner side of its bottom
        return [PointLight((0.5, 9.0, 0.4), Color.rgb(1.0, 1.0, 1.0), 3.0)]
    key = PointLight((1.5, 9.0, 2.0), Color.rgb(1.0, 1.0, 1.0), 3.0)
    if kind == "L1":
        return [key]
    sun = DirectionalLight((-0.6, -2.0, -0.4), Color(1.0, 0.95, 0.8, 1.0), 0.4)
    sun.direction = vec3(-0.6, -2.0, -0.4)  # (the constructor normalises)
    return [key, AmbientLight.default_ambient(), sun, PointLight((-4.0, 6.0, 3.0), Color.rgb(0.6, 0.7, 1.0), 2.0)]


def camera(w, h):
    cam = Camera.new_perspective(to_radians(50.0), f32(w) / f32(h), 0.1, 100.0)
    cam.transform.position = vec3(0.0, 7.0, 11.0)
    cam.look_at((0.0, 0.5, 0.0))
    return cam


def config(w, h, mode="lambert_shadow", max_depth=1):
    return RaytracerConfig(max_depth=max_depth, samples_per_pixel=1, width=w, height=h, jitter="center", mode=mode,
                           background_color=Color(0.1, 0.1, 0.15, 1.0))


def _filler(k, count, mat_a, mat_b):
    a = 2.0 * math.pi * (k + 0.5) / count
    c = (5.5 * math.cos(a), 0.22, 5.5 * math.sin(a))
    if k % 5 == 2:
        return SDFObject(SDFBox(c, (0.4, 0.44, 0.4)), mat_b)
    return Sphere(c, 0.22, mat_a)


def objects(n, occ, sdf_occluder):
    """n objects; the occluder at index `occ` (n >= 2: the ground at index 0, so occ >= 1)."""
    ground = LambertianMaterial(Color.rgb(0.5, 0.5, 0.5))
    red = LambertianMaterial(Color.rgb(0.7, 0.3, 0.3))
    blue = LambertianMaterial(Color.rgb(0.3, 0.4, 0.7))
    green = LambertianMaterial(Color.rgb(0.3, 0.7, 0.3))
    if n == 1:
        return [SDFObject(SDFRing((0.0, 2.5, 0.0), 2.0, 0.5), red)]
    assert 1 <= occ < n
    occluder = (SDFObject(SDFSphere((0.0, 2.2, 0.0), 0.9), red) if sdf_occluder else Sphere((0.0, 2.2, 0.0), 0.9, red))
    objs, k = [], 0
    for i in range(n):
        if i == 0:
            objs.append(Sphere((0.0, -1000.0, 0.0), 1000.0, ground))
        elif i == occ:
            objs.append(occluder)
        else:
            objs.append(_filler(k, n - 2, blue, green))
            k += 1
    return objs


def ground_only_objects():
    """17 objects: the ground and 16 small ones huddled in the far left corner of the picture, so that for
    most tiles every light's mask holds the ground alone."""
    ground = LambertianMaterial(Color.rgb(0.5, 0.5, 0.5))
    red = LambertianMaterial(Color.rgb(0.7, 0.3, 0.3))
    green = LambertianMaterial(Color.rgb(0.3, 0.7, 0.3))
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, ground)]
    for k in range(16):
        c = (-4.5 + 0.5 * (k % 4), 0.2 + 0.45 * (k // 8), -3.0 + 0.5 * ((k // 4) % 2))
        objs.append(SDFObject(SDFSphere(c, 0.2), green) if k % 4 == 1 else Sphere(c, 0.2, red))
    return objs


def _placements(n):
    """Occluder indices: the first and the last slot of the second group, and the last index overall."""
    out = [i for i in (GROUP, 2 * GROUP - 1) if 1 <= i < n - 1]
    return out + [n - 1]


# (id, objects, lights): the object counts 1, 2, group - 1 / group / group + 1, 17, 31, 32, 33, 64, 65, the
# three placements at 17 objects / 4 lights and 33 / 1, one and four lights, and both sides of
# num_prims * num_lights <= 64 (shadow_cull_lanes up to it -- 16 x 4, 33 x 1, 64 x 1 -- shadow_cull past it
# -- 17 x 4, 32 x 4, 65 x 1).
def _cases():
    out = [("n1-L1", lambda: objects(1, 0, True), "ring")]
    plan = [(2, "L4", None), (GROUP - 1, "L1", None), (GROUP, "L4", None), (GROUP + 1, "L1", None), (16, "L4", None),
            (17, "L4", "all"), (17, "L1", None), (31, "L1", None), (32, "L4", None), (33, "L1", "all"), (64, "L1", None),
            (65, "L1", None)]
    seen = set()
    for n, lk, sweep in plan:
        if n < 2:
            continue
        for occ in (_placements(n) if sweep else [n - 1]):
            cid = f"n{n}-{lk}-occ{occ}"
            if cid in seen:
                continue
            seen.add(cid)
            out.append((cid, (lambda n=n, occ=occ: objects(n, occ, (n + occ) % 2 == 1)), lk))
    out.append(("ground-only-L4", ground_only_objects, "L4"))
    return out


CASES = _cases()
CASE_BY_ID = {c[0]: c for c in CASES}
