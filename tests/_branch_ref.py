"""Host-side reference of one DMC branching step and the constructed clone
patterns of tests/test_gpu_dmc_tiles.py (checked against the oracle, without a
GPU, in tests/test_branch_ref.py).

The device branches in tiles of 1024 parents (four per thread,
csrc/qmc_kernels_misc.h); which kernels run is decided by max_num_walkers
alone:

    max_num_walkers   nblocks   path
    <= 1024           1         branch_fused_kernel, one tile
    1025 .. 2048      2         branch_fused_kernel, two tiles walked serially
    > 2048            >= 3      branch_count_kernel + branch_scatter_kernel
                                (+ dmc_finish_kernel / dmc_local_sums_kernel
                                summing block_esum)

The reference below is the rule itself (qmc_base/dmc.py:638-653):
kids = min(floor(w + u), maxw), the table lists every parent `kids` times in
parent order and is cut at maxw.

Weights come from WEIGHTS and uniforms from UNIFORMS only, so w + u stays at
least 0.125 away from every integer: the device keeps log-weights, and its
exp(log w) round trip (one or two ulp) cannot change a count.
"""
import math

import numpy as np

TILE = 1024
WEIGHTS = (0.0, 0.25, 0.5, 1.0, 1.5, 2.25, 3.5)
UNIFORMS = (0.125, 0.375, 0.625, 0.875)
# (w, u) pairs of the two sets by the clone count floor(w + u) they give
COMBOS = {}
for _w in WEIGHTS:
    for _u in UNIFORMS:
        COMBOS.setdefault(int(math.floor(_w + _u)), []).append((_w, _u))
MAX_KIDS = max(COMBOS)          # 4

# (max_num_walkers, parents): both sides of every tile edge, parent counts
# that are not multiples of the four parents a thread owns, under each cap
CAPS = (1024, 2048, 2049, 5000)
PARENTS = (1023, 1024, 1025, 2047, 2049, 4097)
SHAPES = [(m, p) for m in CAPS for p in PARENTS if p <= m]


def nblocks(maxw):
    return (int(maxw) + TILE - 1) // TILE


def path_name(maxw):
    nb = nblocks(maxw)
    return f'fused, {nb} tile(s)' if nb <= 2 else f'multi-block, {nb} tiles'


def branch_reference(weight, uniform, maxw):
    """-> (kids[P], table[n_w]) of one branching step."""
    w = np.asarray(weight, dtype=np.float64)
    u = np.asarray(uniform, dtype=np.float64)
    kids = np.minimum(np.floor(w + u), float(maxw)).astype(np.int64)
    table = np.repeat(np.arange(w.size, dtype=np.int64), kids)[:int(maxw)]
    return kids, table


def energy_sum_and_bound(energy, table):
    """E_t = fsum(E_parent(table)) and the bound on a fixed-order fp64 sum of
    at most n_w products: 2 * n_w * 2^-53 * sum |E_parent(table)|."""
    e = np.asarray(energy, dtype=np.float64)[table]
    bound = 2.0 * len(table) * 2.0 ** -53 * math.fsum(np.abs(e))
    return math.fsum(e), bound


def _draw(kids, rng):
    """Weights / uniforms from the two sets that give the clone counts."""
    w, u = np.zeros(len(kids)), np.zeros(len(kids))
    for s, k in enumerate(kids):
        w[s], u[s] = COMBOS[int(k)][rng.randint(len(COMBOS[int(k)]))]
    return w, u


def _background(count, rng):
    return rng.choice([0, 1, 2], size=count, p=[0.3, 0.4, 0.3]).astype(np.int64)


def _with_sum(count, total, rng):
    """`count` clone counts in 0..MAX_KIDS that add up to `total` exactly."""
    assert 0 <= total <= MAX_KIDS * count, (count, total)
    kids = np.full(count, total // count, dtype=np.int64)
    kids[rng.choice(count, total - int(kids.sum()), replace=False)] += 1
    for a, b in rng.randint(count, size=(2 * count, 2)):
        if a != b and kids[a] < MAX_KIDS and kids[b] > 0:
            kids[a] += 1
            kids[b] -= 1
    assert int(kids.sum()) == total
    return kids


def _below(kids, total, rng, keep=()):
    """Thin `kids` out (never the indices in `keep`) until the sum is at most
    `total`."""
    kids = kids.copy()
    free = np.setdiff1d(np.nonzero(kids)[0], np.asarray(keep, dtype=np.int64))
    for s in rng.permutation(free):
        if int(kids.sum()) <= total:
            break
        kids[s] = 0
    assert int(kids.sum()) <= total
    return kids


def pattern_names(maxw, parents):
    return [name for name, _ in _patterns(maxw, parents, None)]


def pattern(maxw, parents, name):
    """-> (weight[P], uniform[P]) of the named pattern."""
    rng = np.random.RandomState(
        [int(maxw), int(parents), sum(map(ord, name))])
    for nm, make in _patterns(maxw, parents, rng):
        if nm == name:
            return make()
    raise KeyError(name)


def _patterns(M, P, rng):
    """[(name, maker)] of the patterns that exist for cap M and P parents."""
    edges = [e for e in range(TILE, P, TILE)]     # first parents of tiles 1..
    last = P - 1
    out = []

    def add(name, kids_fn, big=None):
        def make():
            kids = kids_fn()
            w, u = _draw(kids, rng)
            if big is not None:
                w[big[0]] = big[1]
            return w, u
        out.append((name, make))

    # random counts, nothing arranged (cut at the cap where they exceed it)
    add('background', lambda: _background(P, rng))

    if edges:
        # the last parent of a tile has four children, the first of the next
        # tile none -- and the reverse; total kept under the cap
        def rich_last(rev):
            def f():
                kids = _background(P, rng)
                keep = []
                for e in edges:
                    kids[e - 1], kids[e] = (0, 4) if rev else (4, 0)
                    keep += [e - 1, e]
                return _below(kids, M, rng, keep)
            return f
        add('tile_last_rich_next_first_none', rich_last(False))
        add('tile_last_none_next_first_rich', rich_last(True))

    if P > 2 * TILE:
        # whole tiles of parents without children (tile total 0) between
        # productive ones: tiles 1, 3, ...
        def empty_tiles():
            kids = _background(P, rng)
            for t in range(1, (P - 1) // TILE, 2):
                kids[t * TILE:(t + 1) * TILE] = 0
            kids[last] = 3
            return _below(kids, M, rng, [last])
        add('empty_tile_between', empty_tiles)

    def only_last():
        kids = np.zeros(P, dtype=np.int64)
        kids[last] = 4
        return kids
    add('all_from_last_parent', only_last)

    # the cap inside one parent's children: sum(kids[:j]) = M - 2, parent j
    # has four, the parents after it (which have children too) appear nowhere
    j = -(-(M - 2) // 3) + 1
    if j % 4 == 0:
        j += 1
    j = min(j, P - 2)
    if j > 0 and MAX_KIDS * j >= M - 2:
        def cap_mid(j=j):
            kids = np.r_[_with_sum(j, M - 2, rng), 4,
                         1 + _background(P - j - 1, rng)]
            return kids
        add('cap_inside_one_parents_children', cap_mid)

    # the cap on the first child of a tile: the tiles before parent e fill the
    # table exactly (tile offset == M), and one short of it (only the first
    # child of the tile fits)
    full = [e for e in edges if MAX_KIDS * e >= M]
    if full:
        e = full[0]

        def cap_tile(short, e=e):
            def f():
                kids = np.r_[_with_sum(e, M - short, rng),
                             1 + _background(P - e, rng)]
                kids[e] = 3
                return kids
            return f
        add('cap_at_first_child_of_tile', cap_tile(0))
        add('cap_after_first_child_of_tile', cap_tile(1))

    # the children fill the table exactly: no truncation, last child of the
    # last parent in slot M - 1
    if MAX_KIDS * (P - 1) >= M - 2 and M - 2 >= 0:
        add('cap_equals_total',
            lambda: np.r_[_with_sum(P - 1, M - 2, rng), 2])

    # one parent with more children than the cap: it fills the table from its
    # offset to the cap, the parents after it appear nowhere
    jb = TILE - 1 if P > TILE else P // 2

    def before_big():
        kids = 1 + _background(P, rng)
        kids[:jb] = _below(_background(jb, rng), M - 1, rng)
        return kids
    add('one_parent_1e6', before_big, big=(jb, 1e6))
    add('one_parent_1e300', before_big, big=(jb, 1e300))
    return out
