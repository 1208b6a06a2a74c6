"""The triangle table of the device mesher (sdf-viewer_amd/csrc/mc_table.inc) is generated, not copied: the committed
file must be what tools/gen_mc_table.py produces, and the table must triangulate ANY sign field into a closed,
consistently oriented surface (checked on random fields, where every ambiguous face and case shows up)."""
import numpy as np

from mesh_ref import directed_edges, mc_generator as load_generator   # the one loader of tools/gen_mc_table.py


def test_committed_table_is_the_generated_one():
    gen = load_generator()
    with open(gen.OUT) as f:
        assert f.read() == gen.render(gen.build())


def test_table_basics():
    table = load_generator().build()
    assert len(table) == 256 and table[0] == [] and table[255] == []
    assert max(len(t) for t in table) == 5
    for case, tris in enumerate(table):
        crossing = {e for e in range(12) if ((case >> load_generator().edge_ends(e)[0]) & 1) != ((case >> load_generator().edge_ends(e)[1]) & 1)}
        used = {e for t in tris for e in t}
        assert used == crossing, case   # every crossing edge carries a vertex, no other does


def test_random_sign_fields_give_closed_oriented_surfaces():
    gen = load_generator()
    table = gen.build()
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = 5
        inside = np.zeros((n + 1, n + 1, n + 1), bool)
        inside[1:-1, 1:-1, 1:-1] = rng.random((n - 1, n - 1, n - 1)) < (0.5 if trial % 2 else 0.25)
        vid, idx = {}, []                                 # vertex ids of the (lattice point, axis) keys, and the triangles
        for k in range(n):
            for j in range(n):
                for i in range(n):
                    case = 0
                    for c in range(8):
                        if inside[i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)]:
                            case |= 1 << c
                    for tri in table[case]:
                        for e in tri:
                            a, s = divmod(e, 4)
                            others = [b for b in range(3) if b != a]
                            owner = [i, j, k]
                            owner[others[0]] += s & 1
                            owner[others[1]] += s >> 1
                            idx.append(vid.setdefault((tuple(owner), a), len(vid)))
        directed = directed_edges(idx)
        assert directed, "the random field has a surface"
        assert all(c == 1 for c in directed.values())
        assert all((v, u) in directed for (u, v) in directed), "open edge: the surface is not watertight"
