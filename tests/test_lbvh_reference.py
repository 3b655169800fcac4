"""tests/lbvh_reference.py on its own, without a device: the reference the GPU tests hold the LBVH builder to must not be trusted
merely because the kernels agree with it.  Its trees are proper on every input class of the GPU tests, a grid comes out in Z-order
(computed here from the integer cells, not from the keys), equal keys keep ascending triangle index, and the chain is 64 deep."""
import numpy as np
import pytest

import lbvh_reference as lr

CLASSES = {
    **{f"random-{n}": (lambda n=n: lr.random_triangles(n)) for n in (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513)},
    **{f"degenerate-{k}": (lambda k=k: lr.degenerate(k)) for k in ("plane", "line", "point")},
    "5x8000": lambda: lr.repeated(5, 8000),
    "1x4099": lambda: lr.repeated(1, 4099),
    "chain": lr.chain,
    "random-65537": lambda: lr.random_triangles(65537),
    "extremes-xyz": lambda: lr.range_extremes(axes=3),
    "extremes-xy": lambda: lr.range_extremes(axes=2),
    "grid": lambda: lr.grid()[0],
    "non-finite": lr.non_finite,
}


@pytest.mark.parametrize("name", list(CLASSES))
def test_reference_tree_is_proper(name):
    tris = lr.pack(CLASSES[name]())
    nodes = lr.reference_nodes(tris)
    lr.check_tree(nodes, tris, boxes=name != "non-finite")
    assert not lr.padding_words(nodes).any()


def test_demo_scene_reference_tree_is_proper():
    from mi3pt_host import scenes
    tris = scenes.demo_scene().triangles
    lr.check_tree(lr.reference_nodes(tris), tris)


def test_grid_leaves_come_in_z_order():
    pos, ijk = lr.grid()
    tris = lr.pack(pos)
    got = lr.leaves_in_order(lr.reference_nodes(tris))

    def z(cell):                                         # x highest, from the integer coordinates alone
        return sum(((int(cell[a]) >> b) & 1) << (3 * b + 2 - a) for a in range(3) for b in range(3))

    assert got == sorted(range(len(ijk)), key=lambda t: z(ijk[t]))
    assert len({z(c) for c in ijk}) == 512


def test_equal_keys_keep_ascending_triangle_index():
    tris = lr.pack(lr.repeated(5, 40))
    keys = lr.morton_keys(tris)
    assert len(set(keys)) == 5 and all(keys[i] == keys[i % 5] for i in range(200))
    leaves = lr.leaves_in_order(lr.reference_nodes(tris))
    assert [keys[t] for t in leaves] == sorted(keys)
    for k in set(keys):
        run = [t for t in leaves if keys[t] == k]
        assert len(run) == 40 and run == sorted(run)


def test_chain_is_64_levels_deep():
    tris = lr.pack(lr.chain())
    keys = lr.morton_keys(tris)
    assert sorted(keys) == [0] + [1 << b for b in range(63)] + [(1 << 63) - 1]
    assert lr.depth(lr.reference_nodes(tris)) == 64


def test_one_and_two_triangles():
    tris = lr.pack(lr.random_triangles(1))
    nodes = lr.reference_nodes(tris)
    assert len(nodes) == 1 and lr.depth(nodes) == 1
    p = np.stack([tris["aPosition"], tris["bPosition"], tris["cPosition"]], 1)[0]
    assert (nodes["isLeaf"][0], nodes["left"][0], nodes["right"][0], nodes["triangleIndex"][0]) == (1, -1, -1, 0)
    assert np.array_equal(nodes["min"][0], p.min(0)) and np.array_equal(nodes["max"][0], p.max(0))
    tris = lr.pack(lr.random_triangles(2))
    nodes = lr.reference_nodes(tris)
    assert len(nodes) == 3 and lr.depth(nodes) == 2
    assert nodes["isLeaf"].tolist() == [0, 1, 1] and (nodes["left"][0], nodes["right"][0], nodes["triangleIndex"][0]) == (1, 2, -1)
    assert sorted(nodes["triangleIndex"][1:].tolist()) == [0, 1]


def test_quantisation_edges():
    """extent 0 -> cell 0; the largest centroid lands in the top cell 2^21 - 1, not in 2^21; NaN centroids do not move the bounds"""
    cen = np.array([[0.0, 5.0, np.nan], [1.0, 5.0, 2.0], [0.5, 5.0, 4.0], [np.nan, 5.0, 3.0]], np.float32)
    q = lr.quantise(cen)
    assert q[:, 0].tolist() == [0, (1 << 21) - 1, 1 << 20, 0]
    assert q[:, 1].tolist() == [0, 0, 0, 0]
    assert q[:, 2].tolist() == [0, 0, (1 << 21) - 1, 1 << 20]
    assert lr.interleave(*(np.array([v], np.uint64) for v in (1, 0, 0))).tolist() == [4]
    assert lr.interleave(*(np.array([v], np.uint64) for v in (0, 1 << 20, 1))).tolist() == [(1 << 61) | 1]
