"""The integer core of the device BVH build (rrte_amd/csrc/mesh_build.hpp: Morton code, cell, Karras'
range and split search, the parent walk) without a GPU: tests/cpp/lbvh_host_check.cpp, a stand-alone
program built with -fsanitize=address,undefined, runs exactly those functions and must agree with the
independent top-down restatement in tests/lbvh_ref.py on every link, parent and depth."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lbvh_ref as lr

ROOT = Path(__file__).resolve().parents[1]
F = np.float32


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lbvh") / "lbvh_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "lbvh_host_check.cpp")], check=True)
    return exe


def _run(tool, text):
    r = subprocess.run([str(tool)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.split("\n")


def _keys_of_codes(codes):
    """Leaf keys of leaves whose first slots have the ascending `codes`."""
    return [(int(c) << 32) | j for j, c in enumerate(sorted(int(c) for c in codes))]


def caterpillar_codes(cluster_leaves):
    """One leaf in each Morton cell 2^k, k = 0..29, one in the far corner, `cluster_leaves` in cell 0."""
    return [0] * cluster_leaves + [1 << k for k in range(30)] + [(1 << 30) - 1]


def _key_sets():
    rng = np.random.default_rng(20240607)
    sets = {f"random{n}": _keys_of_codes(rng.integers(0, 1 << 30, n)) for n in (1, 2, 3, 5, 64, 257)}
    sets["random64dups"] = _keys_of_codes(rng.integers(0, 7, 64))  # runs of equal codes among distinct ones
    sets["equal37"] = _keys_of_codes([0x2AAAAAAA] * 37)
    sets["two_codes"] = _keys_of_codes([5] * 6 + [0x3000000A] * 4)
    sets["caterpillar1"] = _keys_of_codes(caterpillar_codes(1))
    sets["caterpillar8"] = _keys_of_codes(caterpillar_codes(8))
    return sets


KEY_SETS = _key_sets()


@pytest.mark.parametrize("name", list(KEY_SETS))
def test_host_program_and_reference_agree(tool, name):
    keys = KEY_SETS[name]
    n = len(keys)
    out = _run(tool, "K %d %s\n" % (n, " ".join(str(k) for k in keys)))
    assert out[0] == f"tree {n}"
    t = lr.tree(keys)
    lr.check_tree(keys, t)
    recs = [list(map(int, line.split()[1:])) for line in out if line.startswith("rec ")]
    leaves = [list(map(int, line.split()[1:])) for line in out if line.startswith("leaf ")]
    assert len(recs) == max(n - 1, 0) and len(leaves) == (n if n > 1 else 0)
    for i, (idx, c0, c1, axis, parent, depth, first, last) in enumerate(recs):
        assert idx == i
        assert [c0, c1] == t["child"][i], (i, c0, c1, t["child"][i])
        assert (axis, parent, depth) == (t["axis"][i], t["parent"][i], t["depth"][i]), i
        assert (first, last) == t["span"][i] and 0 <= axis <= 2
    for j, (idx, parent) in enumerate(leaves):
        assert idx == j and parent == t["leaf_parent"][j]
    if n > 1:
        assert recs[0][4] == -1 and sum(r[4] == -1 for r in recs) == 1  # record 0 is the only root
        assert max(r[5] for r in recs) + 1 == t["depth_max"]


def test_equal_codes_split_by_position_near_balance():
    t = lr.tree(KEY_SETS["equal37"])
    assert t["depth_max"] == 6 and set(t["axis"]) == {0}  # ceil(log2(37)) records on the longest path


def test_caterpillar_depths_straddle_the_traversal_stack():
    assert lr.tree(KEY_SETS["caterpillar1"])["depth_max"] == 30 <= lr.MAX_RECORDS
    assert lr.tree(KEY_SETS["caterpillar8"])["depth_max"] == 33 > lr.MAX_RECORDS


def test_morton_codes(tool):
    cases = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1023, 1023, 1023), (512, 0, 0), (0, 0, 512), (5, 3, 6), (682, 341, 1023)]
    want = [0, 4, 2, 1, (1 << 30) - 1, 1 << 29, 1 << 27, None, None]
    # (5, 3, 6): x = 101, y = 011, z = 110 -> triples (x y z) from the top bit: 101 011 110
    want[7] = 0b101011110
    # x = 1010101010, y = 0101010101, z all ones -> triples 101 011 101 011 ...
    want[8] = int("101011" * 5, 2)
    assert lr.morton(cases) == want
    out = _run(tool, "".join("M %d %d %d\n" % c for c in cases))
    assert [int(line.split()[1]) for line in out if line.startswith("morton")] == want


def _bits(x):
    return int(np.array([x], F).view(np.uint32)[0])


def test_cells_on_hand_computed_points(tool):
    # centroid box [-1, 3] x [2, 2] x [-0.0, 8]: ext 4, 0 and 8
    lo, hi = np.array([-1.0, 2.0, -0.0], F), np.array([3.0, 2.0, 8.0], F)
    c = np.array([[-1.0, 2.0, -0.0],     # the low corner: cell 0 on every axis (z: -0.0 - -0.0 = +0)
                  [3.0, 2.0, 8.0],       # the high corner: 1024 clamps to 1023; y has no extent
                  [1.0, 2.0, 4.0],       # the middle: 512
                  [0.0, 2.0, 0.0078125],  # x (1 / 4) * 1024 = 256; z 1 / 1024 of the extent: exactly cell 1
                  [2.99999976, 2.0, 0.0078124995]], F)  # just below the corner: 1023; just below cell 1: 0
    want = [[0, 0, 0], [1023, 0, 1023], [512, 0, 512], [256, 0, 1], [1023, 0, 0]]
    assert lr.cells(c, lo, hi).tolist() == want
    ext = (hi - lo).astype(F)
    lines = "".join("C %d %d %d\n" % (_bits(p[a]), _bits(lo[a]), _bits(ext[a])) for p in c for a in range(3))
    got = [int(line.split()[1]) for line in _run(tool, lines) if line.startswith("cell")]
    assert np.array(got).reshape(-1, 3).tolist() == want
    # no extent on any axis: everything is cell 0, code 0
    one = np.array([[4.0, -2.0, 0.5]] * 3, F)
    assert lr.cells(one, one[0], one[0]).tolist() == [[0, 0, 0]] * 3
    got = [int(line.split()[1]) for line in _run(tool, "C %d %d %d\n" % (_bits(4.0), _bits(4.0), _bits(0.0))) if line]
    assert got == [0]


def test_range_of_duplicates_and_of_five_triangles():
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [5.0, 5.0, 5.0], [6.0, 5.0, 5.0], [5.0, 6.0, 5.0]], F)
    dup = lr.build_range(pos, np.array([[0, 1, 2]] * 9))
    assert dup["codes"] == [0] * 9 and dup["order"].tolist() == list(range(9)) and len(dup["links"]) == 2 and dup["depth"] == 2
    five = lr.build_range(pos, np.array([[3, 4, 5], [0, 1, 2], [3, 4, 5], [0, 1, 2], [0, 1, 2]]), slot_base=10, rec_base=7)
    assert five["order"].tolist() == [1, 3, 4, 0, 2] and five["root"] == 7 and five["depth"] == 1
    assert five["links"].tolist() == [[lr.LEAF_BIT | (3 << 24) | 10, lr.LEAF_BIT | (0 << 24) | 14]]
    assert lr.build_range(pos, np.array([[0, 1, 2]] * 3), slot_base=6)["root"] == lr.LEAF_BIT | (2 << 24) | 6
    assert lr.build_range(pos, np.zeros((0, 3), np.int64))["root"] == lr.LEAF_BIT
