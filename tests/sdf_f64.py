"""An independent float64 reference of the build-defined SDF path, the fourth pin of
the oracle.

Written from the formulas of DESIGN.md §6, not from the device code, the C oracle or
tests/numpy_ref.py: positions are (n, 3) float64 arrays with named columns, every deformer is a
rotation or a scaling of that vector about a named axis (one explicit right-handed 2-D rotation per
axis, no index arithmetic), and sin/cos are numpy's.  It can therefore disagree with the three
bit-for-bit restatements, which share one shape.

What is taken from elsewhere, and why: value noise is defined by its integer lattice hash, so the
lattice values (one hash per corner, three channels cut from its bits, one seed per octave) come from
numpy_ref -- integer arithmetic, exact -- and only the fade and the trilinear blend are done here.

`evaluate(program, points)` runs a lowered node program (LoweredScene.nodes) at float64 points.
`classify_rays` samples a ray at a fixed spacing and sorts it into solid / clear / undecided.

`quirks` describes the shape deliberately wrongly (tests/test_sdf_f64_cpu.py 'the checker bites');
the library is never touched by it.
"""
from collections import namedtuple

import numpy as np

import numpy_ref
from rrte_amd import abi

X, Y, Z = 0, 1, 2
AXIS_NAME = {0: "x", 1: "y", 2: "z"}

Node = namedtuple("Node", "op f i")

# deliberately wrong descriptions
QUIRK_SIN_SIGN = "sine sign flipped"
QUIRK_SWAP_UW = "u/w swapped"
QUIRK_SDIFF = "smooth difference as smin(a, -b)"


def program(nodes, first=0, count=None):
    """A lowered program as plain records: parameters are the stored float32 values, taken exactly."""
    count = len(nodes) - first if count is None else count
    return [Node(int(n.op), [float(v) for v in n.f], [int(v) for v in n.i]) for n in nodes[first:first + count]]


def length(*cols):
    out = np.abs(cols[0])
    for c in cols[1:]:
        out = np.hypot(out, c)
    return out


# ------------------------------------------------------------------------------------- leaves
def _capped(d_radial, d_axial):
    """Exact distance to a solid of revolution whose section is the quadrant d_radial, d_axial <= 0."""
    outside = length(np.maximum(d_radial, 0.0), np.maximum(d_axial, 0.0))
    return outside + np.minimum(np.maximum(d_radial, d_axial), 0.0)


def _segment_distance(px, py, ax, ay, bx, by):
    ex, ey = bx - ax, by - ay
    t = np.clip(((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    return np.hypot(px - (ax + ex * t), py - (ay + ey * t))


def leaf(op, f, p):
    q = p - np.array(f[0:3])
    x, y, z = q[:, X], q[:, Y], q[:, Z]
    if op == abi.SDF_SPHERE:
        return length(x, y, z) - f[3]
    if op == abi.SDF_BOX:  # full extents f[4:7]
        d = np.abs(q) - 0.5 * np.array(f[4:7])
        return length(*np.maximum(d, 0.0).T) + np.minimum(d.max(axis=1), 0.0)
    if op == abi.SDF_CYLINDER:  # radius, height about Y
        return _capped(np.hypot(x, z) - f[3], np.abs(y) - 0.5 * f[4])
    if op == abi.SDF_PRISM:
        tri = np.maximum(np.abs(x) * 0.866025 + y * 0.5, -y) - f[5] / 4.0
        return np.maximum(np.abs(z) - f[6] / 2.0, tri)
    if op == abi.SDF_TORUS:  # ring in XZ
        return np.hypot(np.hypot(x, z) - f[3], y) - f[4]
    if op == abi.SDF_TUBE:  # outer, inner, height
        wall = np.abs(np.hypot(x, z) - 0.5 * (f[3] + f[4])) - 0.5 * (f[3] - f[4])
        return _capped(wall, np.abs(y) - 0.5 * f[5])
    if op == abi.SDF_RING:  # ring in XY
        return np.hypot(np.hypot(x, y) - f[3], z) - f[4]
    if op == abi.SDF_CONE:
        # section in (rho, y): the triangle (0, -h/2), (r, -h/2), (0, +h/2); distance to its base and
        # to its slanted side, negative between them
        r, hh = f[3], 0.5 * f[4]
        rho = np.hypot(x, z)
        base = _segment_distance(rho, y, 0.0, -hh, r, -hh)
        side = _segment_distance(rho, y, r, -hh, 0.0, hh)
        # inside: above the base and on the axis side of the slanted line through (r, -hh), (0, hh)
        inside = (y > -hh) & (y < hh) & (rho * (2.0 * hh) < r * (hh - y))
        return np.where(inside, -1.0, 1.0) * np.minimum(base, side)
    if op == abi.SDF_CAPSULE:  # segment on Y
        hh = 0.5 * f[4]
        return length(x, y - np.clip(y, -hh, hh), z) - f[3]
    if op == abi.SDF_ELLIPSOID:
        r = np.array(f[4:7])
        k0 = length(*(q / r).T)
        k1 = length(*(q / (r * r)).T)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(k1 > 0.0, k0 * (k0 - 1.0) / k1, -np.min(r))
    raise NotImplementedError(op)


def ellipsoid_k1(f, p):
    q = p - np.array(f[0:3])
    r = np.array(f[4:7])
    return length(*(q / (r * r)).T)


# ---------------------------------------------------------------------------------------- CSG
def smooth_min(a, b, k):
    h = np.clip(0.5 + 0.5 * (b - a) / k, 0.0, 1.0)
    return b + (a - b) * h - k * h * (1.0 - h)


def combine(op, a, b, k, quirks=()):
    if op == abi.SDF_UNION:
        return np.minimum(a, b)
    if op == abi.SDF_DIFFERENCE:
        return np.maximum(a, -b)
    if op == abi.SDF_INTERSECTION:
        return np.maximum(a, b)
    if op == abi.SDF_SMOOTH_UNION:
        return smooth_min(a, b, k)
    if op == abi.SDF_SMOOTH_DIFFERENCE:
        if QUIRK_SDIFF in quirks:
            return smooth_min(a, -b, k)
        return -smooth_min(-a, b, k)
    if op == abi.SDF_SMOOTH_INTERSECTION:
        return -smooth_min(-a, -b, k)
    raise NotImplementedError(op)


# ---------------------------------------------------------------------------------- deformers
def _rotate_about_x(q, angle, quirks):
    s, c = _sin(angle, quirks), np.cos(angle)
    y, z = q[:, Y], q[:, Z]
    if QUIRK_SWAP_UW in quirks:
        y, z = z, y
    return np.stack([q[:, X], c * y - s * z, s * y + c * z], axis=1)


def _rotate_about_y(q, angle, quirks):
    s, c = _sin(angle, quirks), np.cos(angle)
    z, x = q[:, Z], q[:, X]
    if QUIRK_SWAP_UW in quirks:
        z, x = x, z
    return np.stack([s * z + c * x, q[:, Y], c * z - s * x], axis=1)


def _rotate_about_z(q, angle, quirks):
    s, c = _sin(angle, quirks), np.cos(angle)
    x, y = q[:, X], q[:, Y]
    if QUIRK_SWAP_UW in quirks:
        x, y = y, x
    return np.stack([c * x - s * y, s * x + c * y, q[:, Z]], axis=1)


ROTATE = {"x": _rotate_about_x, "y": _rotate_about_y, "z": _rotate_about_z}
# the unit vector of an axis, and the mask of the two coordinates across it
ALONG = {"x": np.array([1.0, 0.0, 0.0]), "y": np.array([0.0, 1.0, 0.0]), "z": np.array([0.0, 0.0, 1.0])}


def _sin(angle, quirks):
    return -np.sin(angle) if QUIRK_SIN_SIGN in quirks else np.sin(angle)


def _fbm3(xs, octaves, persistence, seed):
    """Three-channel fractal value noise: octave o has weight persistence^o, frequency 2^o and its own
    seed; each is a trilinear blend of the eight lattice corners with the smoothstep fade."""
    total = np.zeros_like(xs)
    weight, scale = 1.0, 1.0
    for o in range(octaves):
        sx = xs * scale
        cell = np.floor(sx)
        t = sx - cell
        fade = t * t * (3.0 - 2.0 * t)
        ic = cell.astype(np.int64)
        oct_seed = (seed + o * 0x85EBCA6B) & 0xFFFFFFFF
        for cx in (0, 1):
            wx = fade[:, X] if cx else 1.0 - fade[:, X]
            for cy in (0, 1):
                wy = fade[:, Y] if cy else 1.0 - fade[:, Y]
                for cz in (0, 1):
                    wz = fade[:, Z] if cz else 1.0 - fade[:, Z]
                    h = numpy_ref._lattice_hash(ic[:, X] + cx, ic[:, Y] + cy, ic[:, Z] + cz, oct_seed)
                    w = wx * wy * wz
                    for ch in range(3):
                        total[:, ch] += weight * w * numpy_ref._channel(h, ch).astype(np.float64)
        weight *= persistence
        scale *= 2.0
    return total


def deform(node, p, quirks=()):
    pivot = np.array(node.f[0:3])
    q = p - pivot
    if node.op == abi.SDF_TWIST:
        axis = AXIS_NAME[node.i[0]]
        q = ROTATE[axis](q, node.f[3] * (q @ ALONG[axis]), quirks)
    elif node.op == abi.SDF_BEND:
        axis, direction = AXIS_NAME[node.i[0]], AXIS_NAME[node.i[1]]
        q = ROTATE[axis](q, node.f[3] * (q @ ALONG[direction]), quirks)
    elif node.op == abi.SDF_TAPER:
        # t runs from 0 to 1 over [-length/2, +length/2] along the axis; the two coordinates across
        # the axis are divided by lerp(start, end, t)
        axis = ALONG[AXIS_NAME[node.i[0]]]
        start, end, span = node.f[3], node.f[4], node.f[5]
        t = np.clip((q @ axis + 0.5 * span) / span, 0.0, 1.0)
        s = start + (end - start) * t
        q = q * axis + (q * (1.0 - axis)) / s[:, None]
    elif node.op == abi.SDF_NOISE:
        frequency, amplitude, persistence = node.f[3], node.f[4], node.f[5]
        q = q + amplitude * _fbm3(q * frequency, node.i[0], persistence, node.i[1])
    elif node.op == abi.SDF_WAVE:
        axis, displaced = ALONG[AXIS_NAME[node.i[0]]], ALONG[AXIS_NAME[node.i[1]]]
        q = q + displaced * (node.f[3] * _sin(node.f[4] * (q @ axis), quirks))[:, None]
    else:
        raise NotImplementedError(node.op)
    return q + pivot


# ---------------------------------------------------------------------------------- programs
def evaluate(prog, points, quirks=(), singular=None):
    """The postfix program at (n, 3) float64 points: a leaf pushes its value, a CSG op replaces the two
    top values a (below) and b (top) by op(a, b), a deformer saves the point and replaces it, POP_POINT
    restores the saved one.  `singular`, a bool array, collects where a definition is singular
    (ellipsoid k1 < 1e-3, a NaN operand)."""
    p = np.asarray(points, np.float64)
    values, saved = [], []
    for nd in prog:
        if nd.op < abi.SDF_UNION:
            v = leaf(nd.op, nd.f, p)
            if singular is not None:
                if nd.op == abi.SDF_ELLIPSOID:
                    singular |= ellipsoid_k1(nd.f, p) < 1e-3
                singular |= np.isnan(v)
            values.append(v)
        elif nd.op < abi.SDF_BEND:
            b = values.pop()
            a = values.pop()
            values.append(combine(nd.op, a, b, nd.f[0], quirks))
        elif nd.op < abi.SDF_POP_POINT:
            saved.append(p)
            p = deform(nd, p, quirks)
        else:
            p = saved.pop()
    assert len(values) == 1 and not saved
    return values[0]


def evaluate_chunked(prog, points, quirks=(), chunk=1 << 18):
    points = np.asarray(points, np.float64)
    out = np.empty(len(points))
    for s in range(0, len(points), chunk):
        out[s:s + chunk] = evaluate(prog, points[s:s + chunk], quirks)
    return out


def gradient(prog, points, h, quirks=()):
    """Normalised central-difference gradient at step h."""
    g = np.empty((len(points), 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        g[:, k] = evaluate(prog, points + e, quirks) - evaluate(prog, points - e, quirks)
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def grid(center, half, n):
    ax = np.linspace(-half, half, n)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return g + np.asarray(center, np.float64)


def farthest_inside(prog, center, half, n):
    """(distance from `center` of the farthest grid point with F <= 0, that point, the number of such
    points, and their bounding box) on an n^3 grid of half-width `half`."""
    pts = grid(center, half, n)
    inside = pts[evaluate_chunked(prog, pts) <= 0.0]
    if len(inside) == 0:
        return 0.0, None, 0, None
    d = np.linalg.norm(inside - np.asarray(center, np.float64), axis=1)
    k = int(np.argmax(d))
    return float(d[k]), inside[k], len(inside), (inside.min(axis=0), inside.max(axis=0))


# --------------------------------------------------------------------------------------- rays
SOLID, CLEAR, UNDECIDED = 1, 0, -1


def classify_rays(prog, origins, directions, t_min, t_max, center, r_test, margin, spacing, quirks=(),
                  rays_per_chunk=128):
    """Samples F(o + t d) at `spacing` over the part of [t_min, t_max] within r_test of `center`.
    Returns (kind, t_solid, t_cross): kind SOLID where some sample has F < -margin, CLEAR where every
    sample has F > +margin (a ray that never comes within r_test is clear), else UNDECIDED; t_solid is
    the first solid sample's t and t_cross the first sample's with F <= 0 (inf where there is none)."""
    o = np.asarray(origins, np.float64)
    d = np.asarray(directions, np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    n = len(o)
    oc = o - np.asarray(center, np.float64)
    b = (oc * d).sum(1)
    disc = b * b - ((oc * oc).sum(1) - r_test * r_test)
    root = np.sqrt(np.maximum(disc, 0.0))
    lo = np.maximum(np.broadcast_to(np.asarray(t_min, np.float64), (n,)), -b - root)
    hi = np.minimum(np.broadcast_to(np.asarray(t_max, np.float64), (n,)), -b + root)
    live = (disc > 0.0) & (hi > lo)
    kind = np.full(n, CLEAR, np.int8)
    t_solid = np.full(n, np.inf)
    t_cross = np.full(n, np.inf)
    steps = int(np.ceil(2.0 * r_test / spacing)) + 1
    ks = np.arange(steps) * spacing
    for s in range(0, n, rays_per_chunk):
        idx = np.flatnonzero(live[s:s + rays_per_chunk]) + s
        if idx.size == 0:
            continue
        t = lo[idx, None] + ks[None, :]
        valid = t <= hi[idx, None]
        tt = np.minimum(t, hi[idx, None])  # the last sample sits on the interval's end
        pts = o[idx, None, :] + tt[..., None] * d[idx, None, :]
        f = evaluate(prog, pts.reshape(-1, 3), quirks).reshape(tt.shape)
        valid |= np.roll(valid, 1, axis=1) & ~valid  # keep the one clamped sample at the end
        solid = (f < -margin) & valid
        clear = ((f > margin) | ~valid).all(axis=1)
        any_solid = solid.any(axis=1)
        first = np.argmax(solid, axis=1)
        kind[idx] = np.where(any_solid, SOLID, np.where(clear, CLEAR, UNDECIDED))
        t_solid[idx] = np.where(any_solid, tt[np.arange(len(idx)), first], np.inf)
        below = (f <= 0.0) & valid
        t_cross[idx] = np.where(below.any(axis=1), tt[np.arange(len(idx)), np.argmax(below, axis=1)], np.inf)
    return kind, t_solid, t_cross


def tetrahedral_normal(prog, points, h, quirks=()):
    """Normalised sum of k_i F(p + h k_i) over the four tetrahedral taps."""
    g = np.zeros((len(points), 3))
    for k in ((1, -1, -1), (-1, -1, 1), (-1, 1, -1), (1, 1, 1)):
        k = np.array(k, np.float64)
        g += k * evaluate(prog, points + h * k, quirks)[:, None]
    return g / np.linalg.norm(g, axis=1, keepdims=True)
