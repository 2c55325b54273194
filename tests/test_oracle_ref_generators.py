"""The REFERENCE generators (tst/laplacian, tst/heat, tst/graph getInput plugins) against the oracle's restatement AND the
product's vectorised generators: same elements, same order, same element matrices.  The reference's output is the
recorded golden tests/golden/ref_generators.npz (tests/golden/make_ref_generator_goldens.py records it from the plugins
that oracle/ref_build/Makefile compiles into oracle/_ref); where those plugins are built, every case also checks that they
still return the golden, bit for bit."""
import os

import numpy as np
import pytest

from geneo4petsc_amd import decomp
from oracle import driver_oracle as drv
from oracle import ref_generators as rg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_generators.npz")

GRID = [("laplacian", "--size 5 --dim 3 --kappa 2. lin", dict(size=5, dim=3, kappa_max=2.0, interp="lin")),
        ("laplacian", "--size 7 --dim 2 --weakScaling 2", dict(size=7, dim=2, weak=2)),
        ("laplacian", "--size 6 --dim 1 --inpEps 0.01 --kappa 5 quad",
         dict(size=6, dim=1, inp_eps=0.01, kappa_max=5.0, interp="quad")),
        ("laplacian", "--size 10 --dim 3 --kappa 2. lin", dict(size=10, dim=3, kappa_max=2.0, interp="lin")),
        ("heat", "--size 4 --dim 3 --kappa 100 minmax --lbd 2. --dt 0.5",
         dict(size=4, dim=3, kappa_max=100.0, interp="minmax", heat=True, lbd=2.0, dt=0.5)),
        ("heat", "--size 5 --dim 3 --kappa 2. quad --lbd 1. --dt 0.1",
         dict(size=5, dim=3, kappa_max=2.0, interp="quad", heat=True, lbd=1.0, dt=0.1)),
        ("heat", "--size 6 --dim 2", dict(size=6, dim=2, heat=True))]
GRAPH = [("--size 9 --level 2", dict(size=9, level=2)),
         ("--size 16 --level 1 --noGround", dict(size=16, level=1, no_ground=True)),
         ("--size 10 --level 2 --noGround", dict(size=10, level=2, no_ground=True)),
         ("--size 4 --level 3 --weakScaling 4 --inpEps 0.1", dict(size=4, level=3, weak=4, inp_eps=0.1))]


def golden_key(plugin, args):
    return plugin + " " + args


def golden_cases():
    """(plugin, args) of every case, args exactly as handed to the plugin"""
    return [(p, a) for p, a, _ in GRID] + [("graph", a.replace(" ", "#")) for a, _ in GRAPH]


def _golden(plugin, args):
    g = np.load(GOLDEN)
    i = [str(k) for k in g["keys"]].index(golden_key(plugin, args))
    ne, nn = (int(v) for v in g["c%d_dims" % i])
    ptr = [int(v) for v in g["c%d_ptr" % i]]
    mat = g["c%d_mat" % i]
    m = drv.Mesh(ne, nn, ptr, [int(v) for v in g["c%d_idx" % i]], [])
    pos = 0
    for e in range(ne):
        k = ptr[e + 1] - ptr[e]
        m.elemSubMat.append([float(v) for v in mat[pos:pos + k * k]])
        pos += k * k
    return m


def _reference(plugin, args):
    ref = _golden(plugin, args)
    if rg.available():
        live = rg.get_input(plugin, args)
        assert (live.nbElem, live.nbNode) == (ref.nbElem, ref.nbNode)
        assert live.elemPtr[:live.nbElem + 1] == ref.elemPtr and live.elemIdx == ref.elemIdx
        assert [list(v) for v in live.elemSubMat] == ref.elemSubMat
    return ref


def _same_as_oracle(ref, orc):
    assert (ref.nbElem, ref.nbNode) == (orc.nbElem, orc.nbNode)
    assert ref.elemPtr[:ref.nbElem + 1] == orc.elemPtr[:orc.nbElem + 1] and ref.elemIdx == orc.elemIdx
    for a, b in zip(ref.elemSubMat, orc.elemSubMat):
        np.testing.assert_allclose(a, b, rtol=1e-15, atol=0)


def _same_as_product(ref, pm):
    assert (ref.nbElem, ref.nbNode) == (pm.nbElem, pm.nbNode)
    for e in range(ref.nbElem):
        s, t = ref.elemPtr[e], ref.elemPtr[e + 1]
        nn = t - s
        assert list(pm.nodes[e][:nn]) == ref.elemIdx[s:t]
        np.testing.assert_allclose(pm.mats[e].reshape(2, 2)[:nn, :nn].ravel(), ref.elemSubMat[e], rtol=1e-15)


@pytest.mark.parametrize("plugin,args,kw", GRID, ids=[g[1] for g in GRID])
def test_grid_generators(plugin, args, kw):
    ref = _reference(plugin, args)
    _same_as_oracle(ref, drv.grid_input(**kw))
    _same_as_product(ref, decomp.grid_mesh(**kw))


@pytest.mark.parametrize("args,kw", GRAPH, ids=[g[0] for g in GRAPH])
def test_graph_generator(args, kw):
    ref = _reference("graph", args.replace(" ", "#"))     # '#' separators as on the reference CLI
    _same_as_oracle(ref, drv.graph_input(**kw))
    _same_as_product(ref, decomp.graph_mesh(**kw))
