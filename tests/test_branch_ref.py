"""Pins the branching reference of tests/_branch_ref.py (what
tests/test_gpu_dmc_tiles.py trusts on the GPU) to the oracle, without a GPU:
the same constructed clone patterns through `oracle.DmcEnsemble.step` with the
weights written into its `prev_weight` buffer and the uniforms as tape."""
from math import pi

import numpy as np
import pytest

from . import _branch_ref as br

CASES = [(m, p, name) for m, p in br.SHAPES
         for name in br.pattern_names(m, p)]
N = 8


def model(oracle):
    from phd_qmclib_amd.mrbp_qmc import Spec
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=N, supercell_size=N,
                tbf_contact_cutoff=0.25 * N)
    return oracle.model_from_cfc(spec.cfc_spec)


def oracle_branching_step(oracle, m, pos, weight, uniform, maxw):
    """One oracle step that only branches (time step 1e-300, zero normals)
    -> (yield, ensemble)."""
    P = len(pos)
    orc = oracle.DmcEnsemble(m, pos, 1e-300, maxw, P, 0.5, seed=1,
                             nthreads=oracle.max_threads())
    orc.bufs['prev_weight'][:P] = weight
    out = orc.step(np.r_[uniform, np.zeros(8)], np.zeros(maxw * N))
    return out, orc


def test_patterns_cover_their_edges():
    """The constructed patterns do what their names say (on the reference's
    own counts), every (w, u) comes from the two sets, and every pattern
    exists for at least one shape of each path."""
    seen = {}
    for maxw, P, name in CASES:
        w, u = br.pattern(maxw, P, name)
        assert w.shape == u.shape == (P,)
        assert np.isin(u, br.UNIFORMS).all()
        small = np.isin(w, br.WEIGHTS)
        assert small.sum() >= P - 1
        frac = (w[small] + u[small]) % 1.0
        assert np.all((frac >= 0.125) & (frac <= 0.875))
        kids, table = br.branch_reference(w, u, maxw)
        total, nw = int(kids.sum()), len(table)
        assert 0 < nw <= maxw and nw == min(total, maxw)
        seen.setdefault(name, set()).add(br.nblocks(maxw))
        edges = list(range(br.TILE, P, br.TILE))
        if name == 'tile_last_rich_next_first_none':
            assert all(kids[e - 1] == 4 and kids[e] == 0 for e in edges)
            assert total <= maxw
        elif name == 'tile_last_none_next_first_rich':
            assert all(kids[e - 1] == 0 and kids[e] == 4 for e in edges)
            assert total <= maxw
        elif name == 'empty_tile_between':
            assert not kids[br.TILE:2 * br.TILE].any()
            assert kids[:br.TILE].any() and kids[2 * br.TILE:].any()
        elif name == 'all_from_last_parent':
            assert np.array_equal(table, np.full(4, P - 1))
        elif name == 'cap_inside_one_parents_children':
            j = int(table[-1])
            before = int(kids[:j].sum())
            assert before < maxw < before + kids[j] and nw == maxw
            assert kids[j + 1:].all()
        elif name == 'cap_at_first_child_of_tile':
            e = next(e for e in edges if br.MAX_KIDS * e >= maxw)
            assert kids[:e].sum() == maxw and table[-1] < e
            assert kids[e:].all()
        elif name == 'cap_after_first_child_of_tile':
            e = next(e for e in edges if br.MAX_KIDS * e >= maxw)
            assert kids[:e].sum() == maxw - 1 and table[-1] == e
            assert kids[e] == 3 and kids[e + 1:].all()
        elif name == 'cap_equals_total':
            assert total == maxw and table[-1] == P - 1
        elif name in ('one_parent_1e6', 'one_parent_1e300'):
            j = int(np.nonzero(~small)[0][0])
            off = int(kids[:j].sum())
            assert off < maxw and kids[j] == maxw and kids[j + 1:].all()
            assert np.all(table[off:] == j) and nw == maxw
    for name in ('background', 'all_from_last_parent',
                 'cap_inside_one_parents_children', 'cap_equals_total',
                 'one_parent_1e6', 'one_parent_1e300'):
        assert seen[name] == {1, 2, 3, 5}, (name, seen[name])
    for name in ('tile_last_rich_next_first_none',
                 'tile_last_none_next_first_rich',
                 'cap_at_first_child_of_tile',
                 'cap_after_first_child_of_tile'):
        assert seen[name] >= {2, 3, 5}, (name, seen[name])
    assert seen['empty_tile_between'] == {3, 5}


@pytest.mark.parametrize('maxw,parents,name',
                         [c for c in CASES if c[2] != 'one_parent_1e300'])
def test_branch_reference_vs_oracle(oracle, maxw, parents, name):
    """numpy reference == oracle for every constructed pattern: cloning table,
    population, W_t, E_t (to the fixed-order summation bound), and the
    children carry their parents' configurations and energies.  (The 1e300
    parent is left out: the oracle's integer cast overflows there.)"""
    m = model(oracle)
    pos = N * np.random.RandomState(parents).random_sample((parents, N))
    w, u = br.pattern(maxw, parents, name)
    kids, table = br.branch_reference(w, u, maxw)
    out, orc = oracle_branching_step(oracle, m, pos, w, u, maxw)
    nw = len(table)
    assert out.num_walkers == nw
    assert np.array_equal(orc.cloning_ref[:nw], table)
    assert out.weight == nw
    e_t, bound = br.energy_sum_and_bound(orc.ini_energy, table)
    assert abs(out.energy - e_t) <= bound
    assert np.array_equal(orc.energy[:nw], orc.ini_energy[table])
    assert np.array_equal(orc.confs[:nw], orc.ini_confs[table])
    mask = orc.bufs['actual_mask'].astype(bool)
    assert not mask[:nw].any() and mask[nw:].all()
