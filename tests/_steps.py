"""Helpers shared by the real-step modules (tests/test_gpu_zclass_steps.py:
the position classifier; tests/test_gpu_generic_steps.py: the sine classifier
on generic models): start rows, the oracle's chains and populations yield by
yield, the once-per-walker condition of the sorted-row pair sums.  Nothing
here touches the device."""
import numpy as np

STREAM_DMC_BRANCH = 2           # oracle/qmc_oracle.h: ORC_STREAM_DMC_BRANCH
EDGE_EPS = 1e-6                 # straddling partners: this far from an edge, of L

VMC_W, VMC_YIELDS, VMC_SPREAD = 6, 24, 0.6
DMC_W, DMC_MAXW, DMC_DT, DMC_KAPPA, DMC_STEPS = 12, 16, 5e-4, 0.5, 8


# ---------------------------------------------------------------------------
# configurations
# ---------------------------------------------------------------------------

def jittered_lattice(rng, n, L):
    """A lattice of spacing L / n, every particle displaced by up to 0.3
    spacings: particles spread like an equilibrated walker."""
    return (np.arange(n) + 0.5 + 0.6 * (rng.random_sample(n) - 0.5)) * (L / n)


def straddling_row(rng, n, L, rm):
    """A uniform random row in which chosen particles have partners EDGE_EPS L
    on either side of every edge of the classifier.  Particle 0 at 0.0211 L
    with partners at z0 + s, s = rm -+ eps, (L - rm) -+ eps, L / 2 -+ eps:
    the device sees |z_a - z_b| = s, on the ring the partners at (L - rm) -+
    eps are the ones rm +- eps away on the other side of the particle.  Where
    the row has room (N >= 14) a second particle at 0.9637 L has the mirrored
    partners z1 - s, so both signs of z_a - z_b meet every edge.

    Partners are taken mod L (at a cutoff below 0.0363 L a partner of the
    second particle lies beyond the box boundary: the same distance on the
    ring, which is what the sine classifier sees), and an edge without room
    -- a separation s -+ eps outside (0, L) -- is skipped: its slots keep
    their uniform random positions.  At the cutoffs of the position
    classifier (> 0.45 L) every partner is inside the box as it is."""
    eps = EDGE_EPS * L
    seps = [s + e for s in (rm, L - rm, 0.5 * L) for e in (-eps, eps)
            if s - eps > 0.0 and s + eps < L]
    k = 1 + len(seps)
    row = L * rng.random_sample(n)
    z0, z1 = 0.0211 * L, 0.9637 * L
    row[:k] = np.mod([z0] + [z0 + s for s in seps], L)
    if n >= 14:
        row[7:7 + k] = np.mod([z1] + [z1 - s for s in seps], L)
    assert np.all((row >= 0.0) & (row < L))
    return row


def six_rows(n, L, rm, seed):
    """The rows of part 1: two uniform random rows, one sorted row, one
    jittered lattice, permuted, one row with four particles within 1e-3 of 0
    and of L (on a jittered lattice), one row with pairs straddling the
    classifier's edges.  At rm = L / 2 exactly the edges coincide (the
    straddling partners would sit on top of each other): five rows."""
    rng = np.random.RandomState(seed)
    rows = [L * rng.random_sample(n), L * rng.random_sample(n),
            np.sort(L * rng.random_sample(n)),
            rng.permutation(jittered_lattice(rng, n, L))]
    seam = jittered_lattice(rng, n, L)
    u = 1e-3 * (0.05 + 0.95 * rng.random_sample(4))
    seam[:2], seam[-2:] = u[:2], L - u[2:]
    rows.append(seam)
    if rm != 0.5 * L:
        rows.append(straddling_row(rng, n, L, rm))
    return np.array(rows)


def start_rows(n, L, rm, seed):
    """Six start rows of the trajectories: the rows of part 1 (at rm = L / 2
    a third uniform random row takes the place of the straddling one)."""
    rows = six_rows(n, L, rm, seed)
    if len(rows) < 6:
        rng = np.random.RandomState(seed + 1)
        rows = np.concatenate([rows, L * rng.random_sample((1, n))])
    return rows


def report(part, cid, figures, module='zclass'):
    """One line per test: worst deviations as fractions of their tolerance."""
    print(f'{module} {part} {cid}: ' + ', '.join(
        f'{k} {v:.1e}' if isinstance(v, float) else f'{k} {v}'
        for k, v in figures.items()))


# ---------------------------------------------------------------------------
# VMC
# ---------------------------------------------------------------------------

def oracle_vmc_chains(oracle, m, pos0, spread, seed, nyield, rows=False):
    """The oracle's chains, yield by yield -> (move_stat, energy, log|psi|
    [nyield, W], final positions mod L [W, N], crossings of the box boundary
    counted as in test_long_trajectories_across_the_box_boundary).
    `rows=True` adds the configuration every yield EVALUATES [nyield, W, N]:
    the start row at yield 0, the proposal of yield t >= 1 -- rebuilt from
    the shared Philox move stream as `_traj.vmc_margin` does (word 0 of
    particle i's block moves it)."""
    W, n = pos0.shape
    L = float(m.supercell_size)
    st_o = np.zeros((nyield, W), dtype=bool)
    en_o, wf_o = np.zeros((nyield, W)), np.zeros((nyield, W))
    pos_o = np.zeros((W, n))
    seen = np.zeros((nyield, W, n))
    crossings = 0
    for c in range(W):
        ch = oracle.VmcChain(m, pos0[c], spread, seed=seed, chain=c)
        prev = np.mod(pos0[c], L)
        for t in range(nyield):
            if rows and t == 0:
                seen[t, c] = prev
            elif rows:
                step = int(ch.cfg.step0)
                unit = np.array([oracle.vmc_move_unit(
                    oracle.vmc_move_block(seed, c, step, i)[0])
                    for i in range(n)])
                seen[t, c] = np.mod(ch.pos + unit * spread, L)
            wf, en, st, _ = ch.run(1)
            st_o[t, c], en_o[t, c], wf_o[t, c] = bool(st[0]), en[0], wf[0]
            cur = np.mod(ch.pos, L)
            crossings += int((np.abs(cur - prev) > 0.5 * L).sum())
            prev = cur
        pos_o[c] = np.mod(ch.pos, L)
    out = (st_o, en_o, wf_o, pos_o, crossings)
    return out + (seen,) if rows else out


def _anchor_seam(z, o):
    """`anchor_seam` / `anchor_seam_rows` (qmc_device.h) on the slots o
    (indices into the positions z): the last slot below the first -- a
    particle that crossed the box boundary sits at the wrong end -- rotates
    the row by one slot.  (The first test decides the direction: with two or
    more particles that left through z = 0 in one step the last slot is below
    the SECOND one as well, and the row turns the wrong way, trip after
    trip.)"""
    if z[o[-1]] < z[o[0]]:
        if z[o[-1]] < z[o[1]]:
            return np.concatenate([o[-1:], o[:-1]])
        if z[o[0]] > z[o[-2]]:
            return np.concatenate([o[1:], o[:1]])
    return o


def _exchange(z, o, first):
    """One compare-exchange pass over the slot pairs (first, first + 1),
    (first + 2, first + 3), ..."""
    o = o.copy()
    a = o[first:len(o) - 1:2].copy()
    b = o[first + 1::2][:len(a)].copy()
    sw = z[b] < z[a]
    o[first:len(o) - 1:2] = np.where(sw, b, a)
    o[first + 1::2][:len(a)] = np.where(sw, a, b)
    return o


def sort_slots(z, order):
    """The exact sort of the sorted-row stepping kernels: z -- positions in
    particle order; order -- the particle every slot holds before the sort ->
    (the trips of the kernel's loop until the slots ascend -- 0: they do as
    they come; None: it gave up at its bound and the walker takes the general
    path --, the order it leaves).
      N <= 64         `sort_lanes64` (qmc_sorted64.h): per trip the seam test
                      if an inversion sits at an end of the row, the even pass
                      if a pair (2k, 2k + 1) is inverted, the odd pass if a
                      pair (2k + 1, 2k + 2) is; at most 140 trips;
      N <= 128, even  `sort_rows128` (qmc_sorted128.h), two slots per lane:
                      per trip the seam test, the even phase (the two slots of
                      a lane), the odd phase (across lanes); at most 66."""
    z = np.asarray(z, dtype=np.float64)
    o = np.array(order)
    n = len(o)

    def inverted(o):
        return np.concatenate([[False], z[o[1:]] < z[o[:-1]]])

    inv = inverted(o)
    if not inv.any():
        return 0, o
    if n <= 64:
        for it in range(140):
            if inv[1] or inv[n - 1]:
                o = _anchor_seam(z, o)
            if inv[1::2].any():
                o = _exchange(z, o, 0)
            if inv[2::2].any():
                o = _exchange(z, o, 1)
            inv = inverted(o)
            if not inv.any():
                return it + 1, o
        return None, o
    assert n <= 128 and n % 2 == 0
    for it in range(66):
        o = _exchange(z, _exchange(z, _anchor_seam(z, o), 0), 1)
        if not inverted(o).any():
            return it + 1, o
    return None, o


def general_path_yields(rows, stat, n, L, rm):
    """Where `vmc_step_kernel` increments its counter, for one chain: rows
    [nyield, N] -- the configuration every yield evaluates, particle order;
    stat [nyield] -- the accept series -> (general [nyield]: the yield's walker
    evaluation leaves the sorted-row pair sums, trips [nyield]: of the sort,
    -1 where it gave up).  `fast` is false -- and the model interacting, the
    walker counted -- when
      * N is odd on the (64, 2) shape (no sort is tried), or
      * the exact sort gives up (`sort_slots`), or
      * the ascending row fails the far-partner condition
        (`takes_sorted_rows`);
    (`outside`, a start row with a particle beyond the box, does not occur
    here).  The slots hold the particles in the order the last accepted yield
    after the first left them -- the forced first yield stores nothing --, in
    the order given before that."""
    nyield = len(rows)
    general = np.zeros(nyield, dtype=bool)
    trips = np.zeros(nyield, dtype=int)
    if n > 64 and n % 2:
        general[:] = True
        return general, trips
    order = np.arange(n)
    for t in range(nyield):
        it, after = sort_slots(rows[t], order)
        trips[t] = -1 if it is None else it
        general[t] = it is None or not takes_sorted_rows(rows[t], n, L, rm)
        if t >= 1 and stat[t]:
            order = after
    return general, trips


def far_partner_distances(row, n, L):
    """The distances the once-per-walker condition of the sorted-row pair sums
    compares with L - rm, one per lane in use, as the device forms them on the
    ascending row (qmc_sorted64.h, qmc_sorted128.h):
      N = 64          `far_partner_ok64`: z - z[lane ^ 32], + L in the lower
                      half of the lanes;
      33 <= N <= 63   `far_partner_ok_ring`, nl = N: the partner nl / 2 lanes
                      down the ring, + L when that wraps;
      N = 128         `far_partner_ok128`: own slot 1 against slot 0 of lane
                      gl ^ 32;
      66 <= N <= 126, even: `far_partner_ok_ring128`, nl = N / 2 lanes of two
                      slots."""
    z = np.sort(row)
    if n == 64 or n == 128:
        gl = np.arange(64)
        own, far = (z, z[gl ^ 32]) if n == 64 else \
            (z[2 * gl + 1], z[2 * (gl ^ 32)])
        d = own - far
        d[:32] = d[:32] + L
        return d
    assert 33 <= n <= 63 or (66 <= n <= 126 and n % 2 == 0), n
    nl = n if n < 64 else n // 2
    gl = np.arange(nl)
    src = gl - nl // 2
    wrapped = src < 0
    src = np.where(wrapped, src + nl, src)
    d = z - z[src] if n < 64 else z[2 * gl + 1] - z[2 * src]
    return np.where(wrapped, d + L, d)


def takes_sorted_rows(row, n, L, rm):
    """The once-per-walker condition of the sorted-row pair sums: on the
    ascending row the partner of the last rotation step is closer than L - rm
    for every lane.  A row that fails it is evaluated by the general pair sum
    inside the same kernel, and counted.  An odd N above 64 -- the (64, 2)
    shape without sorted rows: the static test `(n & 1) == 0` of the stepping
    kernels -- never takes them."""
    if n > 64 and n % 2:
        return False
    return bool(np.all(far_partner_distances(row, n, L) < L - rm))


# ---------------------------------------------------------------------------
# DMC
# ---------------------------------------------------------------------------

def dmc_start(n, L, rm, seed):
    """12 walkers: the six start rows twice; in two walkers of the second
    half two particles sit within 5e-3 of 0 and of L (sqrt(2 dt) = 0.03: they
    cross the seam)."""
    pos = np.tile(start_rows(n, L, rm, seed), (2, 1))
    pos[6, :2] = [2e-3, L - 1.5e-3]
    pos[7, :2] = [L - 3e-3, 4e-3]
    return pos


def oracle_prev_weights(orc):
    """The weights the oracle's next branching step reads."""
    maxw = orc.cfg.max_num_walkers
    w = np.ctypeslib.as_array(orc.st.prev_weight, shape=(maxw,))
    return w[:orc.st.prev_num_walkers].copy()


def oracle_dmc_run(oracle, m, pos0, seed, time_step=DMC_DT, tables=None):
    """The oracle's population over DMC_STEPS steps -> (orc, yields, smallest
    distance of a branching w + u from an integer, particles that crossed the
    box boundary).  Asserts that the clone counts rebuilt from the weights
    and the Philox draws ARE the oracle's populations, below the cap.
    `tables`: a list that receives the cloning table of every step."""
    L = float(m.supercell_size)
    orc = oracle.DmcEnsemble(m, pos0, time_step, DMC_MAXW, DMC_W, DMC_KAPPA,
                             seed=seed)
    ys, margin, crossed = [], 1.0, 0
    prev = np.mod(pos0, L)
    for t in range(DMC_STEPS):
        w = oracle_prev_weights(orc)
        assert len(w), 'the population died out'
        u = np.array([oracle.philox_uniform2(seed, s, t, 0,
                                             STREAM_DMC_BRANCH)[0]
                      for s in range(len(w))])
        x = w + u
        margin = min(margin, float(np.abs(x - np.round(x)).min()))
        y = orc.step()
        nw = int(y.num_walkers)
        assert int(np.floor(x).sum()) == nw < DMC_MAXW, t
        cur = np.mod(orc.confs[:nw, 0], L)
        crossed += int((np.abs(cur - prev[orc.cloning_ref[:nw]]) >
                        0.5 * L).sum())
        prev = cur
        ys.append((nw, float(y.energy), float(y.ref_energy)))
        if tables is not None:
            tables.append(orc.cloning_ref[:nw].copy())
    return orc, ys, margin, crossed
